"""Median blur on a real MI355X (-m gpu): mi_blur_enqueue_median / _band, a context given a median by
mi_blur_ctx_set_median, median_blur() and the hosts' --median, byte for byte against a numpy restatement of the definition
in include/mi_blur.h (edge padding, sliding windows, np.partition) and against the CPU device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

pytestmark = pytest.mark.gpu


def ref_median(img, r):
    """img (N, H, W, C) uint8: edge padding by r, every (2r+1)^2 window, the k-th smallest (k = ((2r+1)^2 - 1) / 2)."""
    d = 2 * r + 1
    p = np.pad(img, ((0, 0), (r, r), (r, r), (0, 0)), mode="edge")
    flat = sliding_window_view(p, (d, d), axis=(1, 2)).reshape(img.shape + (d * d,))
    k = (d * d - 1) // 2
    return np.partition(flat, k, axis=-1)[..., k].astype(np.uint8)


def adversarial(rng, n, h, w, c):
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.full((n, h, w, c), 77, np.uint8),
            np.where(rng.random((n, h, w, c)) < 0.5, 0, 255).astype(np.uint8),
            np.where(rng.random((n, h, w, c)) < 0.2, rng.choice([0, 255], (n, h, w, c)), 128).astype(np.uint8),
            rng.choice(np.array([3, 200], np.uint8), (n, h, w, c)),
            rng.choice(np.array([0, 1, 2, 254, 255], np.uint8), (n, h, w, c)),
            np.broadcast_to(((xx * 7 + yy * 3) % 256).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
            np.broadcast_to((((xx + yy) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy()]


@pytest.fixture(scope="module")
def torch_cuda(L):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert L.mi_blur_device_count() >= 1, "libmi_blur.so sees no HIP device"
    torch.cuda.set_device(0)
    return torch


def gpu_median(pkg, L, torch, host, r, offset_in=0, offset_out=0, y0=None, y1=None):
    """host: N x H x W x C -> mi_blur_enqueue_median (or _band for one image with y0/y1), guard bytes around the output."""
    n, h, w, c = host.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size_out = n * (y1 - y0) * w * c
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = L.mi_blur_enqueue_median(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, r, n, s)
    else:
        assert n == 1
        rc = L.mi_blur_enqueue_median_band(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, r, y0, y1, s)
    pkg.check(rc, "mi_blur_enqueue_median")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, y1 - y0, w, c)


# rows of whole 16-byte chunks with 1-4 channels (the fast kernel at radius 1|2) and everything else
ALIGNED = [(2, 64, 80, 3), (1, 40, 64, 4), (3, 33, 16, 1), (1, 100, 1024, 1), (1, 37, 2000, 4), (2, 70, 96, 2),
           (1, 1, 16, 1), (1, 2, 48, 1), (1, 300, 512, 3), (1, 5, 32, 2)]
RAGGED = [(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 31, 29, 2), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3),
          (1, 12, 16, 6), (1, 10, 20, 7), (1, 14, 18, 8)]


def test_enqueue_median_matches_numpy(pkg, L, torch_cuda):
    rng = np.random.default_rng(2024)
    for shapes, aligned in ((ALIGNED, True), (RAGGED, False)):
        for (n, h, w, c) in shapes:
            img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
            for r in range(1, 8):
                got = gpu_median(pkg, L, torch_cuda, img, r)
                kern = "blur_median_fast_kernel" if aligned and r <= 2 else "blur_median_generic_kernel"
                assert L.mi_blur_last_kernel().decode() == kern, ((n, h, w, c), r)
                assert np.array_equal(got, ref_median(img, r)), ((n, h, w, c), r)


def test_enqueue_median_unaligned_pointers(pkg, L, torch_cuda):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 40, 64, 3), dtype=np.uint8)
    for r in (1, 2):
        want = ref_median(img, r)
        assert np.array_equal(gpu_median(pkg, L, torch_cuda, img, r), want)
        assert L.mi_blur_last_kernel() == b"blur_median_fast_kernel"
        for oi, oo in ((1, 0), (0, 7), (3, 5)):
            assert np.array_equal(gpu_median(pkg, L, torch_cuda, img, r, oi, oo), want), (r, oi, oo)
            assert L.mi_blur_last_kernel() == b"blur_median_generic_kernel"


def test_enqueue_median_adversarial(pkg, L, torch_cuda):
    rng = np.random.default_rng(9)
    for (n, h, w, c) in ((1, 48, 64, 3), (2, 20, 48, 4), (1, 19, 16, 1), (1, 19, 30, 3), (1, 13, 11, 5)):
        for img in adversarial(rng, n, h, w, c):
            for r in (1, 2, 3, 7):
                assert np.array_equal(gpu_median(pkg, L, torch_cuda, img, r), ref_median(img, r)), ((n, h, w, c), r)


def test_bands_inside_the_image(pkg, L, torch_cuda):
    rng = np.random.default_rng(12)
    for (h, w, c) in ((64, 80, 3), (37, 17, 3), (50, 64, 4), (40, 48, 1)):
        img = rng.integers(0, 256, size=(1, h, w, c), dtype=np.uint8)
        for r in (1, 2, 4, 7):
            whole = ref_median(img, r)
            for y0, y1 in ((r, h - r), (0, h // 2), (h // 3, h), (5, 6)):
                got = gpu_median(pkg, L, torch_cuda, img, r, y0=y0, y1=y1)
                assert np.array_equal(got, whole[:, y0:y1]), (h, w, c, r, y0, y1)
            for split in (r, h // 2, h - r):                     # a band split with halo r, joined, is the whole image
                top_rows = min(h, split + r)
                top = gpu_median(pkg, L, torch_cuda, np.ascontiguousarray(img[:, :top_rows]), r, y0=0, y1=split)
                b0 = split - r
                bot = gpu_median(pkg, L, torch_cuda, np.ascontiguousarray(img[:, b0:]), r, y0=r, y1=h - b0)
                assert np.array_equal(np.concatenate([top, bot], axis=1), whole), (h, w, c, r, split)


def test_enqueue_median_refusals(pkg, L, torch_cuda):
    d = torch_cuda.zeros(4096, dtype=torch_cuda.uint8, device="cuda")
    p, q = d.data_ptr(), d.data_ptr() + 2048
    for r in (0, 8, -1):
        assert L.mi_blur_enqueue_median(p, q, 16, 8, 3, r, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(p, p, 16, 8, 3, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(p, q, 0, 8, 3, 1, 1, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median_band(p, q, 16, 8, 3, 1, 6, 2, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median_band(p, q, 16, 8, 3, 1, 0, 9, None) == pkg.ERR_INVALID
    assert L.mi_blur_enqueue_median(p, q, 16, 8, 3, 1, 0, None) == pkg.OK


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
    for r in (1, 2):
        pkg.check(L.mi_blur_enqueue_median(d_in.data_ptr(), d_out.data_ptr(), 1024, 1024, 3, r, n, None))
        torch.cuda.synchronize()
        assert L.mi_blur_last_kernel() == b"blur_median_fast_kernel"
        want0 = torch.from_numpy(ref_median(img, r)[0]).cuda()
        for i in (0, n // 2, n - 2):
            assert bool((d_out[i] == want0).all()), (r, i)
        assert np.array_equal(d_out[n - 1].cpu().numpy(), ref_median(last, r)[0]), r
    del d_in, d_out
    torch.cuda.empty_cache()


def test_gpu_and_cpu_agree_on_the_synthetic_stream(pkg, L, torch_cuda):
    n, h, w, c = 1000, 256, 256, 3
    host = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 8)
    for r in (1, 2):
        want = np.empty_like(host)
        pkg.check(L.mi_blur_cpu_run_median(host.ctypes.data, want.ctypes.data, w, h, c, r, n, 16))
        got = gpu_median(pkg, L, torch_cuda, host, r)
        assert np.array_equal(got, want), r


def test_context_with_a_median(pkg, L, torch_cuda):
    """Every submit form of a GPU context takes the median: pageable, pinned (one launch: not the batch server), strided
    bands, one band, planar."""
    rng = np.random.default_rng(21)
    n, h, w, c = 6, 240, 320, 3                                # 1.38 MB of output per submit: the server size class
    img = np.where(rng.random((n, h, w, c)) < 0.1, rng.choice([0, 255], (n, h, w, c)),
                   rng.integers(0, 256, size=(n, h, w, c))).astype(np.uint8)
    isz = img[0].size
    for r in (1, 2, 4):
        want = ref_median(img, r)
        fast = "blur_median_fast_kernel" if r <= 2 else "blur_median_generic_kernel"
        with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
            ctx.set_median(r)
            out = np.zeros_like(img)
            ctx.submit(img.ctypes.data, out.ctypes.data, n)
            ctx.sync()
            assert np.array_equal(out, want)
            assert L.mi_blur_last_kernel().decode() == fast
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
                assert L.mi_blur_last_kernel().decode() == fast
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
            assert L.mi_blur_ctx_set_median(ctx.h, r) == pkg.ERR_STATE
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED


def test_median_blur_python(pkg, torch_cuda):
    rng = np.random.default_rng(30)
    imgs = rng.integers(0, 256, size=(4, 90, 128, 3), dtype=np.uint8)
    for k in (3, 5, 7, 15):
        assert np.array_equal(pkg.median_blur(imgs, k), ref_median(imgs, k // 2)), k
    g = imgs[0, :, :, 0]
    assert np.array_equal(pkg.median_blur(g, 5), ref_median(g[None, :, :, None], 2)[0, :, :, 0])


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


def test_hosts_median_on_the_gpu(pkg, torch_cuda, tmp_path):
    pkg.build_native()
    het, spl = os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")
    rng = np.random.default_rng(40)
    img = np.where(rng.random((240, 320, 3)) < 0.1, rng.choice([0, 255], (240, 320, 3)),
                   rng.integers(0, 256, size=(240, 320, 3))).astype(np.uint8)
    write_ppm(tmp_path / "in.ppm", img)
    for k in (3, 5):
        want = ref_median(img[None], k // 2)[0]
        for mode in ("gpu", "both"):
            out = f"{mode}{k}.ppm"
            r = subprocess.run([het, mode, "0.7", "35", "--image", "in.ppm", "--images", "100", "--median", str(k), "--save", out],
                               cwd=tmp_path, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stdout + r.stderr
            assert f"Blur kernel: {k}x{k} median" in r.stdout
            assert np.array_equal(read_ppm(tmp_path / out), want), (mode, k)
    r = subprocess.run([spl, "0.6", "16", "--image", "in.ppm", "--images", "48", "--median", "5", "--save", "s.ppm"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Halo size: 2 row(s)" in r.stdout and "Blur kernel: 5x5 median" in r.stdout
    assert np.array_equal(read_ppm(tmp_path / "s.ppm"), ref_median(img[None], 2)[0])
