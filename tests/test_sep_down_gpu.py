"""The decimating separable filter on the GPU (mi_blur_enqueue_sep_down, mi_blur_ctx_set_sep_down, the numpy functions,
the hosts' --pyr-down): exact bytes against sep_ref.ref_sep followed by the subsampling (sep_down_ref.py), and which of
the two kernels took each launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from resample_harness import SEP_DOWN, apps, check_gpu_context, check_pointer_offsets, check_synthetic_stream, gpu_run, last, pinned, read_ppm, torch_cuda, write_ppm  # noqa: F401
from sep_down_ref import PRESETS, ref_sep_down
from sep_ref import rand_taps, ref_sep

pytestmark = pytest.mark.gpu

TILED, GENERIC = SEP_DOWN.tiled, SEP_DOWN.generic
PHASES2 = [(2, 2, 0, 0), (2, 2, 1, 0), (2, 2, 0, 1), (2, 2, 1, 1)]
RADII = [(0, 0), (1, 1), (2, 2), (3, 5), (4, 0), (0, 4), (8, 3), (12, 16), (16, 16)]
# blur_sep_down_tiled_kernel's tile (sep_down_kernels.hip, launch_sep_down_tiled; TILE_TH / TILE_NCOLS of kernel_common.h):
# TILE_ROWS input rows x at most TILE_CHUNKS input 16-byte chunk columns, cut in whole groups of 2 chunks (of 6, at most 4 of them, for 3 channels)
TILE_ROWS, TILE_CHUNKS = 32, 32


def tile_chunk_columns(w, c):
    """Input chunk columns per tile strip, as launch_sep_down_tiled cuts them."""
    unit = 6 if c == 3 else 2
    units = w * c // 16 // unit
    nstrips = -(-units // (4 if c == 3 else TILE_CHUNKS // unit))
    return unit * -(-units // nstrips), w * c // 16


def kernel_of(pkg, rng, rx, ry):
    wx, wy = rand_taps(rng, rx), rand_taps(rng, ry)
    return pkg.SepKernel.from_taps(wx, wy), wx, wy


@pytest.mark.parametrize("shape", [(2, 64, 64, 1), (1, 33, 32, 1), (2, 70, 96, 2), (3, 65, 160, 3), (1, 150, 704, 3), (1, 37, 2000, 4), (1, 300, 512, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_aligned_stride_two_takes_the_tiled_kernel(pkg, L, torch_cuda, shape):
    """Stride 2 x 2, all four phases, every radius pair of RADII with fresh asymmetric taps; one restatement per taps."""
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, size=shape, dtype=np.uint8)
    for rx, ry in RADII:
        k, wx, wy = kernel_of(pkg, rng, rx, ry)
        full = ref_sep(img, wx, wy)
        for dec in PHASES2:
            got = gpu_run(SEP_DOWN, pkg, L, torch_cuda, img, (k, dec))
            assert last(L) == TILED, (shape, rx, ry, dec)
            assert np.array_equal(got, full[:, dec[3]::2, dec[2]::2, :]), (shape, rx, ry, dec)


def test_other_shapes_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    for i, shape in enumerate([(1, 17, 33, 3), (2, 30, 250, 3), (1, 9, 5, 1), (1, 50, 7, 5), (1, 24, 64, 5), (1, 1, 1, 3)]):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for j, (rx, ry) in enumerate(RADII):
            k, wx, wy = kernel_of(pkg, rng, rx, ry)
            dec = (2, 2, 0, 0) if shape[1] == 1 else PHASES2[(i + j) % 4]      # phases cycle across the radii; 1 x 1: phase 0 only
            got = gpu_run(SEP_DOWN, pkg, L, torch_cuda, img, (k, dec))
            assert last(L) == GENERIC, (shape, rx, ry, dec)
            assert np.array_equal(got, ref_sep_down(img, wx, wy, *dec)), (shape, rx, ry, dec)
    img = rng.integers(0, 256, size=(2, 70, 96, 2), dtype=np.uint8)             # aligned shape, pointers off 16 bytes
    check_pointer_offsets(SEP_DOWN, pkg, L, torch_cuda, img, (kernel_of(pkg, rng, 3, 5)[0], (2, 2, 1, 1)), offsets=((1, 0), (0, 7)))


def test_other_strides_and_narrow_output_rows(pkg, L, torch_cuda):
    """Bytes only, whichever kernel: output rows that are not whole chunks, and strides other than 2 x 2."""
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, size=(2, 64, 80, 3), dtype=np.uint8)
    for j, (rx, ry) in enumerate(RADII):
        k, wx, wy = kernel_of(pkg, rng, rx, ry)
        dec = PHASES2[j % 4]
        assert np.array_equal(gpu_run(SEP_DOWN, pkg, L, torch_cuda, img, (k, dec)), ref_sep_down(img, wx, wy, *dec)), (rx, ry, dec)
    for shape in ((2, 70, 96, 2), (1, 17, 33, 3)):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        for j, (sx, sy) in enumerate([(1, 1), (2, 1), (1, 2), (3, 3), (4, 4), (4, 2)]):
            rx, ry = RADII[(j + 3) % len(RADII)]
            k, wx, wy = kernel_of(pkg, rng, rx, ry)
            full = ref_sep(img, wx, wy)
            for ox in range(sx):
                for oy in range(sy):
                    got = gpu_run(SEP_DOWN, pkg, L, torch_cuda, img, (k, (sx, sy, ox, oy)))
                    assert np.array_equal(got, full[:, oy::sy, ox::sx, :]), (shape, sx, sy, ox, oy, rx, ry)
            if (sx, sy) == (1, 1):                                           # ... and the bytes of mi_blur_enqueue_sep
                n, h, w, c = shape
                d_in = torch_cuda.from_numpy(img).cuda()
                d_out = torch_cuda.zeros_like(d_in)
                pkg.check(L.mi_blur_enqueue_sep(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), None), "mi_blur_enqueue_sep")
                torch_cuda.cuda.synchronize()
                assert np.array_equal(gpu_run(SEP_DOWN, pkg, L, torch_cuda, img, (k, (1, 1, 0, 0))), d_out.cpu().numpy())


def seam_images(rng, h, w, c):
    """In the manner of filter_harness.seam_image, for this kernel's tiles: low-amplitude noise with 0 / 255 impulses (one
    channel each) and 0 / 255 step edges on both sides of every seam between tiles (input rows and input chunk columns)
    and on the borders; an all-255 image; impulses in the four corners."""
    ncols, cpr = tile_chunk_columns(w, c)
    rows = sorted({0, h - 1} | {y for s in range(TILE_ROWS, h, TILE_ROWS) for y in (s - 2, s - 1, s, s + 1) if y < h})
    cols = sorted({0, w - 1} | {min(max(x + e, 0), w - 1) for s in range(ncols, cpr, ncols) for x in ((s * 16 - 1) // c, -(-s * 16 // c)) for e in (-1, 0, 1)})
    img = rng.integers(118, 139, size=(4, h, w, c), dtype=np.uint8)
    k = 0
    for y in rows:
        for x in cols:
            img[0, y, x, k % c] = 255 if k % 2 else 0
            k += 1
    for s in rows[1:-1:2]:
        img[1, s:, : w // 2] = 255
        img[1, :s, w // 2:] = 0
    for s in cols[1:-1:2]:
        img[1, : h // 3, s:] = 255 - img[1, : h // 3, s:]
    img[2] = 255
    img[3] = 0
    for y in (0, h - 1):
        for x in (0, w - 1):
            img[3, y, x] = 255
    return img


@pytest.mark.parametrize("shape", [(70, 704, 3), (97, 1088, 1), (66, 320, 4)], ids=lambda s: "x".join(map(str, s)))
def test_tile_seams(pkg, L, torch_cuda, shape):
    h, w, c = shape
    rng = np.random.default_rng(7)
    img = seam_images(rng, h, w, c)
    ncols, cpr = tile_chunk_columns(w, c)
    assert cpr > ncols and h > TILE_ROWS                                 # more than one tile both ways
    for r in (1, 7, 16):
        k, wx, wy = kernel_of(pkg, rng, r, r)
        full = ref_sep(img, wx, wy)
        assert (full[2] == 255).all()
        for dec in ((2, 2, 0, 0), (2, 2, 1, 1)):
            got = gpu_run(SEP_DOWN, pkg, L, torch_cuda, img, (k, dec))
            assert last(L) == TILED
            assert (got[2] == 255).all(), (shape, r, dec)
            assert np.array_equal(got, full[:, dec[3]::2, dec[2]::2, :]), (shape, r, dec)


def presets(pkg, L):
    out = []
    for which in PRESETS:
        k, d = pkg.SepKernel(), pkg.Decimation()
        pkg.check(L.mi_blur_sep_down_preset(which, C.byref(k), C.byref(d)), "mi_blur_sep_down_preset")
        out.append((k, (d.sx, d.sy, d.ox, d.oy)))
    return out


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    rng = np.random.default_rng(9)
    check_synthetic_stream(SEP_DOWN, pkg, L, torch_cuda, presets(pkg, L) + [(kernel_of(pkg, rng, 5, 9)[0], (2, 2, 1, 0))])


def test_gpu_context(pkg, L, torch_cuda):
    shape = (6, 240, 320, 3)
    n, h, w, c = shape
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    check_gpu_context(SEP_DOWN, pkg, L, img, presets(pkg, L)[0], TILED)
    # a context without the setter still takes the batch server for the same pinned submit
    with pinned(L, img.size, img.size) as ((pin_in, a), (pin_out, b)), pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as plain:
        a[:] = img.reshape(-1)
        b[:] = 0
        plain.submit(pin_in, pin_out, n)
        plain.sync()
        assert last(L) == "blur_server_kernel"
        box = np.empty_like(img)
        assert L.mi_blur_cpu_run(img.ctypes.data, box.ctypes.data, w, h, c, 1, n, 4) == pkg.OK
        assert np.array_equal(b.reshape(img.shape), box)


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(3, 90, 128, 3), dtype=np.uint8)
    pyr, a2, a4 = (PRESETS[i][0] for i in range(3))
    assert np.array_equal(pkg.pyr_down(stack), ref_sep_down(stack, pyr, pyr))
    assert np.array_equal(pkg.pyr_down(stack[0], batch=1), ref_sep_down(stack[:1], pyr, pyr)[0])
    assert np.array_equal(pkg.area_down(stack, batch=2), ref_sep_down(stack, a2, a2))
    assert np.array_equal(pkg.area_down(stack, 4), ref_sep_down(stack, a4, a4, 4, 4))
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.pyr_down(odd), ref_sep_down(odd[None, :, :, None], pyr, pyr)[0, :, :, 0])


def test_hosts_pyr_down(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    rng = np.random.default_rng(19)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    pyr = PRESETS[0][0]
    want = ref_sep_down(img[None], pyr, pyr)[0]
    for mode in (["gpu", "1.0", "35"], ["both", "0.7", "35"]):
        dst = tmp_path / f"{mode[0]}.ppm"
        r = subprocess.run([het, *mode, "--image", str(src), "--images", "100", "--pyr-down", "--save", str(dst)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Blur kernel: 5x5 pyramid down, 320x240 -> 160x120" in r.stdout
        got = read_ppm(dst)
        assert got.shape == (120, 160, 3) and np.array_equal(got, want), mode
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--pyr-down"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--pyr-down" in r.stdout and "bands are not supported" in r.stdout
    for extra in (["--sigma", "1.0"], ["--median", "3"], ["--resident"], ["--ksize", "5"]):
        r = subprocess.run([het, "gpu", "1.0", "35", "--image", str(src), "--images", "10", "--pyr-down", *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "Error: --pyr-down excludes" in r.stdout, extra
