"""The colour transform on the GPU (mi_blur_enqueue_color, mi_blur_ctx_set_color, cvt_color() and its kin, the hosts'
--color): exact bytes against the numpy restatement of the header's definition (color_ref.py), and which of the two
kernels took each launch."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from color_harness import cpu_run, gpu_run, make_color, preset_color
from color_ref import (BIAS_MAX, GENERIC, PRESETS, ROW_MAX, RUN, TILED, all_colours, blocks, gamma_table, preset, random_transform, ref_color,
                       ref_preset, takes_tiled, threshold_table)
from resample_harness import apps, last, pinned, read_ppm, torch_cuda, write_ppm  # noqa: F401

pytestmark = pytest.mark.gpu

PAIRS = [(c, co) for c in range(1, 5) for co in range(1, 5)]
# (H, W) whose pixel counts bracket the kernel's units: one group; 24 x 2 (rows of 24 C bytes are not whole chunks for
# C = 1 and 3: tiled all the same, the rule is flat); one group below, at and one above a workgroup's run; two
# workgroups plus one group
UNITS = [(4, 4), (2, 24), (RUN - 1, 16), (RUN, 16), (RUN + 1, 16), (2 * RUN + 1, 16)]


def run_tiled(pkg, L, torch, img, k):
    assert takes_tiled(img.shape)
    got = gpu_run(pkg, L, torch, img, k)
    assert last(L) == TILED
    return got


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_every_instance_at_the_kernels_units(pkg, L, torch_cuda, pair):
    c, co = pair
    rng = np.random.default_rng(40 + 10 * c + co)
    for lut_on in (0, 1):
        for i, (h, w) in enumerate(UNITS):
            img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
            assert blocks(2, h, w) == 2 * (1, 1, 1, 1, 2, 3)[i]
            m, bias, shift, lut = random_transform(rng, c, co, lut_on, (0, 16, 7)[i % 3], limit=i % 2 == 0)
            got = run_tiled(pkg, L, torch_cuda, img, make_color(pkg, m, bias, shift, lut))
            assert np.array_equal(got, ref_color(img, m, bias, shift, lut)), (pair, lut_on, h, w)


def test_batches_either_side_of_the_xcd_remap(pkg, L, torch_cuda):
    """Grids of 15 and of 18 workgroups: below 16 the blocks take the runs in order, from 16 on through the XCD remap."""
    h, w, c = 3 * RUN, 16, 3
    assert blocks(1, h, w) == 3
    rng = np.random.default_rng(60)
    k = preset_color(pkg, L, "rgb2ycbcr")
    for n in (5, 6, 11):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        assert (blocks(n, h, w) >= 16) == (n >= 6) and blocks(n, h, w) == 3 * n
        assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, k), ref_preset(img, "rgb2ycbcr")), n


def test_both_ends_of_the_clamp(pkg, L, torch_cuda):
    """Rows that reach -255 * 2^18 - 2^26 and 255 * 2^18 + 2^26, on images of 0 and of 255, at shift 0 and 16; and shift 0
    with small weights, where acc itself is the byte."""
    m = np.array([[ROW_MAX, 0, 0, 0], [-ROW_MAX, 0, 0, 0], [0, ROW_MAX // 2, ROW_MAX // 2, 0], [0, -ROW_MAX // 2, -ROW_MAX // 2, 0]], np.int64)
    bias = np.array([BIAS_MAX, -BIAS_MAX, BIAS_MAX, -BIAS_MAX], np.int64)
    for v in (0, 255):
        img = np.full((1, 8, 8, 3), v, np.uint8)
        acc = np.einsum("oi,i->o", m[:, :3], np.full(3, v, np.int64)) + bias
        if v == 255:
            assert acc.max() == 255 * ROW_MAX + BIAS_MAX and acc.min() == -255 * ROW_MAX - BIAS_MAX
        for shift in (0, 16):
            got = run_tiled(pkg, L, torch_cuda, img, make_color(pkg, m, bias, shift))
            assert np.array_equal(got, ref_color(img, m, bias, shift))
            assert (got[..., 0] == 255).all() and (got[..., 1] == 0).all()
    rng = np.random.default_rng(61)
    img = rng.integers(0, 256, size=(2, 16, 24, 3), dtype=np.uint8)
    m = np.array([[1, 0, 0], [1, 1, 0], [1, 0, -1], [0, 2, -3]], np.int64)
    bias = np.array([0, -100, 50, 128], np.int64)
    got = run_tiled(pkg, L, torch_cuda, img, make_color(pkg, m, bias, 0))
    want = ref_color(img, m, bias, 0)
    assert np.array_equal(got, want) and np.array_equal(got[..., 0], img[..., 0])
    assert (want == 0).any() and (want == 255).any() and len(np.unique(want[..., 1:])) > 150


def test_all_colours_round_trip(pkg, L, torch_cuda):
    """All 2^24 colours through RGB2YCBCR, then YCBCR2RGB on the result, both through the tiled kernel."""
    img = all_colours()
    ycc = run_tiled(pkg, L, torch_cuda, img, preset_color(pkg, L, "rgb2ycbcr"))
    assert np.array_equal(ycc, ref_preset(img, "rgb2ycbcr"))
    back = run_tiled(pkg, L, torch_cuda, ycc, preset_color(pkg, L, "ycbcr2rgb"))
    assert np.array_equal(back, ref_preset(ycc, "ycbcr2rgb"))
    assert np.abs(back.astype(np.int16) - img.astype(np.int16)).max() <= 1


def test_tables(pkg, L, torch_cuda):
    rng = np.random.default_rng(62)
    img = rng.integers(0, 256, size=(2, 30, 40, 3), dtype=np.uint8)
    m, bias, shift = preset("rgb2ycbcr")
    per = np.stack([rng.permutation(256) for _ in range(3)]).astype(np.uint8)       # a different permutation per channel
    assert not np.array_equal(per[0], per[1]) and not np.array_equal(per[1], per[2])
    assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, make_color(pkg, m, bias, shift, per)), ref_color(img, m, bias, shift, per))
    # the same launch with lut_on = 0 ignores a garbage table
    assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, make_color(pkg, m, bias, shift, per, lut_on=0)), ref_color(img, m, bias, shift))
    eye = np.eye(3, dtype=np.int64)
    for table in (threshold_table(100), threshold_table(-1, 3, 200), gamma_table(2.2), gamma_table(0.45)):
        lut = np.stack([table] * 3)
        assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, make_color(pkg, eye, [0, 0, 0], 0, lut)), table[img])


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    """W * H not a multiple of 16; an aligned shape with a pointer off 16 bytes."""
    rng = np.random.default_rng(63)
    for h, w in ((7, 5), (1, 1), (3, 17)):
        for c, co in ((3, 1), (1, 3), (4, 4), (2, 3), (3, 4)):
            img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
            assert not takes_tiled(img.shape)
            for lut_on in (0, 1):
                m, bias, shift, lut = random_transform(rng, c, co, lut_on, 16, limit=False)
                got = gpu_run(pkg, L, torch_cuda, img, make_color(pkg, m, bias, shift, lut))
                assert last(L) == GENERIC, (h, w, c, co)
                assert np.array_equal(got, ref_color(img, m, bias, shift, lut)), (h, w, c, co, lut_on)
    img = rng.integers(0, 256, size=(2, 35, 96, 3), dtype=np.uint8)
    for name in ("rgb2gray", "rgb2rgba"):
        k, want = preset_color(pkg, L, name), ref_preset(img, name)
        assert np.array_equal(run_tiled(pkg, L, torch_cuda, img, k), want)
        for off in ((1, 0), (0, 7), (8, 0), (0, 8), (7, 1)):
            assert not takes_tiled(img.shape, *off)
            assert np.array_equal(gpu_run(pkg, L, torch_cuda, img, k, *off), want), off
            assert last(L) == GENERIC, off


def test_image_offsets_are_64_bit(pkg, L, torch_cuda):
    """3 images of 16384 x 16384 x 4 -> 1 channel: 3 GiB in, so the third image starts beyond 2^31.  Filled on the device
    with a tiled 4096-byte pattern plus the image index; the first and last 4 rows of every image are compared."""
    torch = torch_cuda
    free, _ = torch.cuda.mem_get_info()
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of free device memory, {free >> 20} MiB are free")
    n, h, w, c = 3, 16384, 16384, 4
    isz = h * w * c
    pattern = ((np.arange(4096, dtype=np.int64) * 37 + (np.arange(4096) >> 5) * 11) % 251).astype(np.uint8)
    d_pat = torch.from_numpy(pattern).cuda()
    d_in = torch.empty(n * isz, dtype=torch.uint8, device="cuda")
    for i in range(n):
        d_in[i * isz:(i + 1) * isz].view(-1, 4096)[:] = d_pat + i
    d_out = torch.full((n * h * w + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    m, bias = np.array([[30000, -20000, 50000, 5536]], np.int64), np.array([1 << 15], np.int64)
    k = make_color(pkg, m, bias, 16)
    pkg.check(L.mi_blur_enqueue_color(d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, C.byref(k), torch.cuda.current_stream().cuda_stream), "mi_blur_enqueue_color")
    torch.cuda.synchronize()
    assert last(L) == TILED
    assert (d_out[n * h * w:] == 0x5A).all().item()
    rows = 4 * w
    for i in range(n):
        for first in (0, h * w - rows):
            src = np.tile(pattern, rows * c // 4096) + np.uint8(i)
            want = ref_color(src.reshape(1, 4, w, c), m, bias, 16)
            got = d_out[i * h * w + first:i * h * w + first + rows].cpu().numpy()
            assert np.array_equal(got, want.reshape(-1)), (i, first)
            assert len(np.unique(want)) > 50
    del d_in, d_out
    torch.cuda.empty_cache()


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    n, h, w, c = 4, 240, 320, 3
    host = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, 4)
    for name, (_, co, _, rows, _) in PRESETS.items():
        if len(rows[0]) != 3:
            continue
        k = preset_color(pkg, L, name)
        want = cpu_run(pkg, L, host, k, 4)
        assert np.array_equal(want, ref_preset(host, name)), name
        assert np.array_equal(run_tiled(pkg, L, torch_cuda, host, k), want), name


@pytest.mark.parametrize("name", ["rgb2gray", "rgb2rgba"])                         # Co < C and Co > C
def test_gpu_context(pkg, L, torch_cuda, name, n_slots=3, repeats=3):
    """A pageable submit, then pinned submits in place over the host link, one launch each (not the batch server); Co > C
    writes more than it reads, so slots sized by the input would be overrun."""
    img = np.random.default_rng(13).integers(0, 256, size=(6, 120, 160, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    want = ref_preset(img, name)
    co = want.shape[-1]
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=n_slots) as ctx:
        k = preset_color(pkg, L, name)
        ctx.set_color(k)
        out = np.full(want.size + 4096, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        t = ctx.sync()
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()
        assert last(L) == TILED
        assert t["bytes_alg"] == n * w * h * (c + co)
        with pinned(L, img.size, want.size + 4096) as ((pin_in, a), (pin_out, b)):
            a[:] = img.reshape(-1)
            z0 = L.mi_blur_zero_copy_launches(ctx.h)
            for r in range(repeats):
                b[:] = 0xA5
                ctx.submit(pin_in, pin_out, n)
                t = ctx.sync()
                assert np.array_equal(b[:want.size].reshape(want.shape), want) and (b[want.size:] == 0xA5).all()
                assert t["bytes_alg"] == (r + 2) * n * w * h * (c + co)
            assert L.mi_blur_zero_copy_launches(ctx.h) == z0 + repeats
            assert last(L) == TILED
            assert L.mi_blur_submit_band(ctx.h, pin_in, pin_out, 60, 2, 2) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_submit_bands(ctx.h, pin_in, pin_out, n, h * w * c, 60, 2, 2) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_submit_planar(ctx.h, pin_in, pin_out, n, 0) == pkg.ERR_UNSUPPORTED
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_ctx_set_color(ctx.h, C.byref(k)) == pkg.ERR_STATE


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(5, 90, 128, 3), dtype=np.uint8)
    assert np.array_equal(pkg.cvt_color(stack, "rgb2gray", batch=2), ref_preset(stack, "rgb2gray"))
    assert np.array_equal(pkg.cvt_color(stack, "rgb2rgba", batch=3), ref_preset(stack, "rgb2rgba"))
    assert np.array_equal(pkg.cvt_color(stack[0], "rgb2ycbcr"), ref_preset(stack[:1], "rgb2ycbcr")[0])
    per = np.stack([rng.permutation(256) for _ in range(3)])
    assert np.array_equal(pkg.apply_lut(stack, per, batch=2), np.stack([per[o][stack[..., o]] for o in range(3)], axis=-1))
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)                        # 3195 pixels: the generic kernel
    assert np.array_equal(pkg.threshold(odd, 99), np.where(odd > 99, 255, 0))
    assert np.array_equal(pkg.gamma_correct(odd, 2.2), gamma_table(2.2)[odd])


def test_hosts_color(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    rng = np.random.default_rng(19)
    img = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    for flag, name, ext in (("gray", "rgb2gray", "pgm"), ("ycbcr", "rgb2ycbcr", "ppm")):
        want = ref_preset(img[None], name)[0]
        for run in (["gpu", "1.0", "35"], ["both", "0.7", "35"], ["cpu", "0", "35"]):
            dst = tmp_path / f"{run[0]}_{flag}.{ext}"
            r = subprocess.run([het, *run, "--image", str(src), "--images", "100", "--color", flag, "--save", str(dst)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Blur kernel: colour transform {flag}, 3 -> {want.shape[-1]} channels" in r.stdout
            if ext == "pgm":
                assert dst.read_bytes() == b"P5\n320 240\n255\n" + want.tobytes(), run
            else:
                assert np.array_equal(read_ppm(dst), want), run
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--color", "gray"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--color" in r.stdout and "bands are not supported" in r.stdout
