"""The remap on the GPU (mi_blur_enqueue_remap, mi_blur_ctx_set_remap, remap() / undistort(), the host's --undistort): exact
bytes against the numpy restatement of the header's definition (remap_ref.py), which of the two kernels took each launch
against the restated eligibility rule, and, through mi_blur_remap_plan (itself checked against the restated walk in
tests/test_remap_host.py), that the maps reach every branch of the tiled kernel: staged, direct and empty tiles."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import warp_perspective_ref as pr
import warp_ref as wr
from filter_harness import apps, read_ppm, torch_cuda, write_ppm  # noqa: F401
from remap_ref import (BARREL_DIST, BILINEAR, CLAMP, CONSTANT, MAPS, MIXED_OUT, MIXED_SHAPE, NEAREST, ONE, affine_map, barrel_K, barrel_map, build_map,
                       cpu_remap_run, gpu_remap_run, identity_map, make_remap, mixed_map, perspective_map, quantise, ref_plan, ref_remap, takes_tiled, tile_geometry)
from test_warp_gpu import TILED_SHAPES, edge_image

pytestmark = pytest.mark.gpu

TILED, GENERIC = "blur_remap_tiled_kernel", "blur_remap_generic_kernel"
BORDERS = (CLAMP, CONSTANT)


def last(L):
    return L.mi_blur_last_kernel().decode()


def blocks(n, wo, ho, c):
    ncols, cpr, rows = tile_geometry(wo, ho, c)
    return n * -(-cpr // ncols) * -(-ho // rows)


def plan(pkg, fmap, shape, border, stage_bytes=0):
    n, h, w, c = shape
    got = pkg.remap_plan(fmap, w, h, c, "bilinear", border, 0, stage_bytes)
    assert got == ref_plan(fmap, w, h, c, BILINEAR, border, stage_bytes)
    return got


@pytest.mark.parametrize("case", TILED_SHAPES, ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1][0]}x{c[1][1]}")
def test_aligned_launches_take_the_tiled_kernel(pkg, L, torch_cuda, case):
    shape, (wo, ho) = case
    n, h, w, c = shape
    assert takes_tiled(shape, wo, ho)
    img = edge_image(np.random.default_rng(sum(shape)), n, h, w, c)
    for name in MAPS:
        fmap = build_map(name, w, h, wo, ho)
        for border in BORDERS:
            p = plan(pkg, fmap, shape, border)
            assert p["tiled"] == 1 and p["direct"] == 0                  # a 96 x 80 input fits the default stage_bytes whole
            if name == "rot30":                                           # all tiles staged, but for the corner tile that CONSTANT finds wholly outside
                assert p["staged"] == p["tiles"] - p["empty"] >= 8 and (border == CONSTANT or p["empty"] == 0)
            if name == "outside":
                assert p["empty"] == (p["tiles"] if border == CONSTANT else 0)
            got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, border, 173)
            assert last(L) == TILED, (name, border)
            assert np.array_equal(got, ref_remap(img, fmap, BILINEAR, border, 173)), (name, border)


@pytest.mark.parametrize("case", TILED_SHAPES, ids=lambda c: "x".join(map(str, c[0])) + f"-{c[1][0]}x{c[1][1]}")
def test_a_small_stage_bytes_takes_both_branches_and_changes_no_byte(pkg, L, torch_cuda, case):
    """stage_bytes = 4096 with rot30 and wild: by the plan both branches occur on every shape (a wild tile's box is the whole
    96 x 80 image, 7680 bytes a channel: direct; one channel's rot30 boxes stay under 4096: staged; with more channels
    rot30 has both in one launch), and the bytes are those of the default."""
    shape, (wo, ho) = case
    n, h, w, c = shape
    img = edge_image(np.random.default_rng(sum(shape) + 1), n, h, w, c)
    staged = direct = 0
    for name in ("rot30", "wild"):
        fmap = build_map(name, w, h, wo, ho)
        for border in BORDERS:
            p = plan(pkg, fmap, shape, border, 4096)
            staged, direct = staged + p["staged"], direct + p["direct"]
            assert name != "wild" or p["direct"] == p["tiles"], (border, p)
            got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, border, 173, stage_bytes=4096)
            assert last(L) == TILED, (name, border)
            assert np.array_equal(got, ref_remap(img, fmap, BILINEAR, border, 173)), (name, border)
    assert staged >= 1 and direct >= 1, (staged, direct)


def test_the_mixed_map_stages_and_samples_directly_in_one_launch(pkg, L, torch_cuda):
    img = np.random.default_rng(8).integers(0, 256, size=MIXED_SHAPE, dtype=np.uint8)
    fmap = mixed_map()
    assert fmap.shape[:2] == MIXED_OUT[::-1]
    for border in BORDERS:
        p = plan(pkg, fmap, MIXED_SHAPE, border)
        assert p["direct"] >= 1 and p["staged"] >= 1 and p["max_box_bytes"] >= 128 * 1024 - 8 * 512
        got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, border, 31)
        assert last(L) == TILED and np.array_equal(got, ref_remap(img, fmap, BILINEAR, border, 31)), border


def test_xcd_remap_on_and_off(pkg, L, torch_cuda):
    """One batch with 16 or more workgroups and one with fewer, every channel count."""
    rng = np.random.default_rng(11)
    for c in (1, 2, 3, 4):
        for n, (h, w), (wo, ho) in ((1, (40, 64), (64, 40)), (3, (80, 96), (144, 70))):
            assert (blocks(n, wo, ho, c) >= 16) == (n == 3)
            img = edge_image(rng, n, h, w, c)
            fmap = affine_map(wr.rotation_m(w, h, 33.0, 1.1), wo, ho)
            got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, CONSTANT, 60)
            assert last(L) == TILED and np.array_equal(got, ref_remap(img, fmap, BILINEAR, CONSTANT, 60)), (c, n)


def test_one_tile_and_narrow_inputs(pkg, L, torch_cuda):
    """Outputs of one chunk (group) per row, one and 33 rows high, and inputs of one chunk per row: the box is the whole row."""
    rng = np.random.default_rng(12)
    for w, c in wr.NARROW_ROWS:                                             # (16, 1), (8, 2), (16, 3), (4, 4): one chunk, or one group of three
        for ho in (1, 33):
            # a narrow OUTPUT of a wider input, and a wide output of the narrow INPUT
            for (wi, hi), wo in (((96, 80), w), ((w, 5), 132 if c == 4 else 144)):
                shape = (2, hi, wi, c)
                img = wr.impulse_rows(rng, *shape)
                for name in ("rot30", "wild", "subpixel", "extremes"):
                    fmap = build_map(name, wi, hi, wo, ho)
                    for border in BORDERS:
                        assert takes_tiled(shape, wo, ho)
                        got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, border, 99)
                        assert last(L) == TILED, (shape, wo, ho, name)
                        assert np.array_equal(got, ref_remap(img, fmap, BILINEAR, border, 99)), (shape, wo, ho, name, border)


def test_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(3)
    # NEAREST on an aligned shape; 5 channels; input rows, then output rows, that are no multiple of 16 bytes; the 1 x 1 cases
    cases = [((2, 80, 96, 4), (132, 70), NEAREST), ((1, 24, 64, 5), (128, 48), BILINEAR), ((1, 17, 33, 3), (48, 29), BILINEAR),
             ((1, 17, 32, 3), (50, 29), BILINEAR), ((1, 1, 1, 3), (9, 9), BILINEAR), ((2, 9, 5, 1), (11, 17), BILINEAR), ((1, 40, 50, 2), (1, 1), NEAREST)]
    for shape, (wo, ho), mode in cases:
        n, h, w, c = shape
        img = edge_image(rng, n, h, w, c)
        for name in ("rot30", "wild", "extremes", "outside"):
            fmap = build_map(name, w, h, wo, ho)
            for border in BORDERS:
                assert not takes_tiled(shape, wo, ho, mode)
                got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, mode, border, 99)
                assert last(L) == GENERIC, (shape, wo, ho, mode)
                assert np.array_equal(got, ref_remap(img, fmap, mode, border, 99)), (shape, name, wo, ho, mode, border)
    # an aligned shape with pointers off 16 bytes, and a map 8 (and 4) bytes off: guards checked inside gpu_remap_run
    img = edge_image(rng, 2, 35, 48, 2)
    fmap = build_map("rot30", 48, 35, 56, 70)
    want = ref_remap(img, fmap, BILINEAR, CONSTANT, 5)
    assert np.array_equal(gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, CONSTANT, 5), want) and last(L) == TILED
    for oi, oo, om in ((1, 0, 0), (0, 7, 0), (3, 5, 0), (0, 0, 8), (0, 0, 4), (7, 3, 8)):
        assert not takes_tiled(img.shape, 56, 70, BILINEAR, oi, oo, om)
        got = gpu_remap_run(pkg, L, torch_cuda, img, fmap, BILINEAR, CONSTANT, 5, 0, oi, oo, om)
        assert np.array_equal(got, want), (oi, oo, om)
        assert last(L) == GENERIC, (oi, oo, om)


def test_equivalences_on_the_gpu(pkg, L, torch_cuda):
    """Every affine and perspective warp is a remap: rot30 and keystone maps give the bytes of the warp launches, the x2
    CLAMP map those of the resize."""
    shape, (wo, ho) = TILED_SHAPES[2]
    n, h, w, c = shape
    img = edge_image(np.random.default_rng(21), n, h, w, c)
    m = wr.rotation_m(w, h, 30.0)
    hm = pr.named_maps(w, h, wo, ho)["keystone"]
    for border in BORDERS:
        got = gpu_remap_run(pkg, L, torch_cuda, img, affine_map(m, wo, ho), BILINEAR, border, 40)
        assert last(L) == TILED
        assert np.array_equal(got, wr.gpu_warp_run(pkg, L, torch_cuda, img, m, wo, ho, BILINEAR, border, 40)) and last(L) == "blur_warp_tiled_kernel"
        got = gpu_remap_run(pkg, L, torch_cuda, img, perspective_map(hm, wo, ho), BILINEAR, border, 40)
        assert last(L) == TILED
        assert np.array_equal(got, pr.gpu_persp_run(pkg, L, torch_cuda, img, hm, wo, ho, BILINEAR, border, 40)) and last(L) == "blur_warp_persp_tiled_kernel"
    img = np.random.default_rng(9).integers(0, 256, size=(2, 45, 64, 3), dtype=np.uint8)
    got = gpu_remap_run(pkg, L, torch_cuda, img, affine_map(wr.scale_matrix(2, 1), 128, 90), BILINEAR, CLAMP)
    assert last(L) == TILED
    assert np.array_equal(got, pkg.resize(img, (128, 90)))
    assert last(L) == "blur_resize_tiled_kernel"


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    shape = (4, 240, 320, 3)
    host = np.empty(shape, np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, 320, 240, 3, 0, 4, 4)
    fmap = barrel_map(320, 240, 320, 240)
    for mode in (BILINEAR, NEAREST):
        want = cpu_remap_run(pkg, L, host, fmap, mode, CONSTANT, 128, 4)
        assert np.array_equal(want, ref_remap(host, fmap, mode, CONSTANT, 128)), mode
        assert np.array_equal(gpu_remap_run(pkg, L, torch_cuda, host, fmap, mode, CONSTANT, 128), want), mode
        assert last(L) == (TILED if mode == BILINEAR else GENERIC)


@pytest.mark.parametrize("target", [(160, 120), (100, 75)], ids=lambda t: "x".join(map(str, t)))
def test_gpu_context(pkg, L, torch_cuda, target):
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = target
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    fmap = barrel_map(w, h, wo, ho)
    want = ref_remap(img, fmap, BILINEAR, CONSTANT, 40)
    kernel = TILED if takes_tiled(shape, wo, ho) else GENERIC
    assert (kernel == TILED) == (target == (160, 120))              # 100 x 3 bytes is no whole number of chunks
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
        mine = fmap.copy()
        ctx.set_remap(make_remap(pkg, wo, ho, BILINEAR, CONSTANT, 40), mine)
        mine[:] = 0x7F7F7F7F                                             # the context copied the map inside the setter
        out = np.full(want.size + 64, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)                  # pageable
        t = ctx.sync()
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()
        assert last(L) == kernel
        assert t["bytes_alg"] == img.size + want.size                   # the map is not counted
        cap = want.size + 4096                                           # pinned, in place, with guard bytes behind the output
        pin_in, pin_out = L.mi_blur_host_alloc(img.size), L.mi_blur_host_alloc(cap)
        try:
            a = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_in)).reshape(img.shape)
            b = np.ctypeslib.as_array((C.c_uint8 * cap).from_address(pin_out))
            a[:] = img
            z0 = L.mi_blur_zero_copy_launches(ctx.h)
            for _ in range(3):
                b[:] = 0xA5
                ctx.submit(pin_in, pin_out, n)
                ctx.sync()
                assert np.array_equal(b[:want.size].reshape(want.shape), want) and (b[want.size:] == 0xA5).all()
            assert L.mi_blur_zero_copy_launches(ctx.h) == z0 + 3
            assert last(L) == kernel
            pitch = w * c
            assert L.mi_blur_submit_band(ctx.h, pin_in, pin_out, 60, 2, 2) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_submit_bands(ctx.h, pin_in, pin_out, n, h * pitch, 60, 2, 2) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_submit_planar(ctx.h, pin_in, pin_out, n, 0) == pkg.ERR_UNSUPPORTED
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_ctx_set_remap(ctx.h, C.byref(make_remap(pkg, wo, ho)), fmap.ctypes.data) == pkg.ERR_STATE
        finally:
            L.mi_blur_host_free(pin_in)
            L.mi_blur_host_free(pin_out)


def test_gpu_context_enlarging(pkg, L, torch_cuda):
    """160 x 120 to 320 x 240: the output is four times the input, so slots sized by the input would be overrun."""
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = 320, 240
    img = np.random.default_rng(14).integers(0, 256, size=shape, dtype=np.uint8)
    fmap = barrel_map(w, h, wo, ho)
    want = ref_remap(img, fmap, BILINEAR, CONSTANT, 40)
    assert want.size == 4 * img.size and takes_tiled(shape, wo, ho)
    assert (want != 40).mean() > 0.5                                     # mostly image, not fill
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=3) as ctx:
        ctx.set_remap(make_remap(pkg, wo, ho, BILINEAR, CONSTANT, 40), fmap)
        cap = want.size + 4096                                           # guard bytes behind the output, pageable and pinned
        out = np.full(cap, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)                  # pageable
        t = ctx.sync()
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()
        assert last(L) == TILED
        assert t["bytes_alg"] == img.size + want.size
        pin_in, pin_out = L.mi_blur_host_alloc(img.size), L.mi_blur_host_alloc(cap)
        try:
            a = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_in)).reshape(img.shape)
            b = np.ctypeslib.as_array((C.c_uint8 * cap).from_address(pin_out))
            a[:] = img
            for k in range(3):
                b[:] = 0xA5
                ctx.submit(pin_in, pin_out, n)
                t = ctx.sync()
                assert np.array_equal(b[:want.size].reshape(want.shape), want) and (b[want.size:] == 0xA5).all()
                assert t["bytes_alg"] == (k + 2) * (img.size + want.size)   # cumulative since the context was made
            assert last(L) == TILED
        finally:
            L.mi_blur_host_free(pin_in)
            L.mi_blur_host_free(pin_out)


def test_two_contexts_keep_their_own_maps(pkg, L, torch_cuda):
    shape = (2, 80, 96, 3)
    n, h, w, c = shape
    img = np.random.default_rng(15).integers(0, 256, size=shape, dtype=np.uint8)
    map_a, map_b = build_map("rot30", w, h, 144, 70), build_map("barrel", w, h, 96, 80)
    want_a, want_b = ref_remap(img, map_a, BILINEAR, CLAMP), ref_remap(img, map_b, BILINEAR, CONSTANT, 7)
    assert not np.array_equal(want_a[:, :70, :96], want_b[:, :70])
    ctx_a, ctx_b = pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=2), pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=2)
    try:
        ctx_a.set_remap(make_remap(pkg, 144, 70, BILINEAR, CLAMP), map_a)
        ctx_b.set_remap(make_remap(pkg, 96, 80, BILINEAR, CONSTANT, 7), map_a[:1, :1].repeat(80, 0).repeat(96, 1))   # replaced at once: its map is freed
        ctx_b.set_remap(make_remap(pkg, 96, 80, BILINEAR, CONSTANT, 7), map_b)
        for _ in range(2):
            out_a, out_b = np.full(want_a.size + 64, 0xA5, np.uint8), np.full(want_b.size + 64, 0xA5, np.uint8)
            ctx_a.submit(img.ctypes.data, out_a.ctypes.data, n)
            ctx_b.submit(img.ctypes.data, out_b.ctypes.data, n)
            ctx_b.sync()
            ctx_a.sync()
            assert np.array_equal(out_a[:want_a.size].reshape(want_a.shape), want_a) and (out_a[want_a.size:] == 0xA5).all()
            assert np.array_equal(out_b[:want_b.size].reshape(want_b.shape), want_b) and (out_b[want_b.size:] == 0xA5).all()
    finally:
        ctx_a.close()
        ctx_b.close()


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(17)
    stack = rng.integers(0, 256, size=(3, 90, 128, 3), dtype=np.uint8)
    xs, ys = rng.uniform(-4, 132, size=(61, 200)), rng.uniform(-4, 94, size=(61, 200))
    fmap = quantise(xs.astype(np.float32), ys.astype(np.float32))
    assert np.array_equal(pkg.remap(stack, xs, ys), ref_remap(stack, fmap))                                     # a float pair
    assert np.array_equal(pkg.remap(stack, fmap, border="clamp", batch=2), ref_remap(stack, fmap, BILINEAR, CLAMP))   # a fixed-point map
    assert np.array_equal(pkg.remap(stack[0], fmap, mode="nearest", fill=200, batch=1), ref_remap(stack[:1], fmap, NEAREST, CONSTANT, 200)[0])
    K = barrel_K(128, 90)
    assert np.array_equal(pkg.undistort(stack, K, BARREL_DIST), ref_remap(stack, pkg.undistort_map(K, BARREL_DIST, (128, 90))))
    odd = rng.integers(0, 256, size=(45, 71), dtype=np.uint8)
    assert np.array_equal(pkg.undistort(odd, barrel_K(71, 45), BARREL_DIST, fill=9),
                          ref_remap(odd[None, :, :, None], pkg.undistort_map(barrel_K(71, 45), BARREL_DIST, (71, 45)), BILINEAR, CONSTANT, 9)[0, :, :, 0])


def test_host_undistort(pkg, apps, torch_cuda, tmp_path):
    het, split = apps
    img = np.random.default_rng(19).integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    fmap = pkg.undistort_map(barrel_K(320, 240), [-0.2, 0, 0, 0, 0], (320, 240))
    for flags, mode, border, fill, name in (([], BILINEAR, CLAMP, 0, "bilinear"), (["--border-fill", "90"], BILINEAR, CONSTANT, 90, "bilinear"),
                                            (["--nearest"], NEAREST, CLAMP, 0, "nearest")):
        want = ref_remap(img[None], fmap, mode, border, fill)[0]
        for run in (["gpu", "1.0", "35"], ["both", "0.7", "35"]):
            dst = tmp_path / f"{run[0]}_{name}_{fill}.ppm"
            r = subprocess.run([het, *run, "--image", str(src), "--images", "100", "--undistort", "-0.2", *flags, "--save", str(dst)],
                               capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            assert f"Blur kernel: {name} remap, undistort k1=-0.2, 320x240 -> 320x240" in r.stdout
            got = read_ppm(dst)
            assert got.shape == (240, 320, 3) and np.array_equal(got, want), (run, name, fill)
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "10", "--undistort", "-0.2"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--undistort" in r.stdout and "bands are not supported" in r.stdout
