"""Rows narrower than the halo on a real MI355X (-m gpu): the one corner of the tile staging the sep, morph, bilateral
and conv kernels share (stage_tile, kernel_common.h) that the tile-edge sweeps of their own test files do not reach.
With 1-3 chunks per row the only strip has halo chunks outside the row on BOTH sides, and the x-clamp fills them from
a row that is the whole tile.  Byte for byte against the library's CPU device."""
import ctypes as C

import numpy as np
import pytest

import conv_ref as cr

pytestmark = pytest.mark.gpu

ROWS = [(16, 1), (32, 1), (8, 2), (16, 3), (4, 4), (8, 4)]      # (w, c): 1, 2, 1, 3, 1, 2 chunks per row
HEIGHTS = (1, 33)                                                # one row; one tile and one row of the next
N = 2


@pytest.fixture(scope="module")
def torch_cuda(L):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert L.mi_blur_device_count() >= 1, "libmi_blur.so sees no HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def images():
    """(w, c, h) -> N x h x w x c random bytes with 0 / 255 impulses in the first and the last pixel of every row."""
    rng = np.random.default_rng(77)
    out = {}
    for w, c in ROWS:
        assert w * c % 16 == 0 and w * c // 16 <= 3
        for h in HEIGHTS:
            img = rng.integers(0, 256, size=(N, h, w, c), dtype=np.uint8)
            flip = (np.arange(N)[:, None] + np.arange(h)[None, :]) % 2 == 1
            img[:, :, 0, :] = np.where(flip, 255, 0)[:, :, None]
            img[:, :, -1, :] = np.where(flip, 0, 255)[:, :, None]
            img.setflags(write=False)
            out[w, c, h] = img
    return out


def rand_taps(rng, r, bits=8):
    cuts = np.sort(rng.integers(0, (1 << bits) + 1, size=2 * r))
    return np.diff(np.concatenate([[0], cuts, [1 << bits]])).tolist()


def sep_filters(pkg, L, rng, r):
    k = pkg.SepKernel.from_taps(rand_taps(rng, r), rand_taps(rng, r))
    yield (lambda i, o, w, h, c, s: L.mi_blur_enqueue_sep(i, o, w, h, c, N, C.byref(k), s),
           lambda i, o, w, h, c: L.mi_blur_cpu_run_sep(i, o, w, h, c, N, C.byref(k), 8))


def morph_filters(pkg, L, rng, r):
    for op in (pkg.MORPH_ERODE, pkg.MORPH_DILATE, pkg.MORPH_GRADIENT):
        yield (lambda i, o, w, h, c, s, op=op: L.mi_blur_enqueue_morph(i, o, w, h, c, op, r, r, N, s),
               lambda i, o, w, h, c, op=op: L.mi_blur_cpu_run_morph(i, o, w, h, c, op, r, r, N, 8))


def bilateral_filters(pkg, L, rng, r):
    k = pkg.Bilateral.gauss(0.0, 25.0, r)
    yield (lambda i, o, w, h, c, s: L.mi_blur_enqueue_bilateral(i, o, w, h, c, N, C.byref(k), s),
           lambda i, o, w, h, c: L.mi_blur_cpu_run_bilateral(i, o, w, h, c, N, C.byref(k), 8))


def conv_filters(pkg, L, rng, r):
    for mode in ("sat", "mag"):                                  # one table and two
        k = cr.make_kernel(pkg, **cr.random_kernel(rng, r, r, mode=mode))
        yield (lambda i, o, w, h, c, s, k=k: L.mi_blur_enqueue_conv(i, o, w, h, c, N, C.byref(k), s),
               lambda i, o, w, h, c, k=k: L.mi_blur_cpu_run_conv(i, o, w, h, c, N, C.byref(k), 8))


# family -> (its tiled kernel, its filters, radius 1 and its largest radius)
FAMILIES = {"sep": ("blur_sep_tiled_kernel", sep_filters, (1, 16)), "morph": ("blur_morph_tiled_kernel", morph_filters, (1, 16)),
            "bilateral": ("blur_bilateral_tiled_kernel", bilateral_filters, (1, 8)), "conv": ("blur_conv_tiled_kernel", conv_filters, (1, 7))}


@pytest.mark.parametrize("family,r", [(f, r) for f, (_, _, radii) in FAMILIES.items() for r in radii])
def test_rows_narrower_than_the_halo(pkg, L, torch_cuda, images, family, r):
    torch = torch_cuda
    kernel, filters, radii = FAMILIES[family]
    assert radii[1] == {"sep": pkg.SEP_MAX_RADIUS, "morph": pkg.MORPH_MAX_RADIUS, "bilateral": pkg.BILATERAL_MAX_RADIUS,
                        "conv": pkg.CONV_MAX_RADIUS}[family]
    rng = np.random.default_rng(1000 + r)
    s = torch.cuda.current_stream().cuda_stream
    for gpu, cpu in filters(pkg, L, rng, r):
        for (w, c, h), img in images.items():
            want = np.empty_like(img)
            pkg.check(cpu(img.ctypes.data, want.ctypes.data, w, h, c), "cpu device")
            d_in = torch.from_numpy(img.copy()).cuda()
            d_out = torch.full((img.size + 128,), 0x5A, dtype=torch.uint8, device="cuda")   # 64 guard bytes either side
            pkg.check(gpu(d_in.data_ptr(), d_out.data_ptr() + 64, w, h, c, s), family)
            torch.cuda.synchronize()
            assert L.mi_blur_last_kernel().decode() == kernel, (w, c, h)
            o = d_out.cpu().numpy()
            assert (o[:64] == 0x5A).all() and (o[64 + img.size:] == 0x5A).all(), ("wrote outside the output", w, c, h)
            assert np.array_equal(o[64:64 + img.size].reshape(img.shape), want), (w, c, h)
