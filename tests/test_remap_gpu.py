"""The remap on the GPU (mi_blur_enqueue_remap, mi_blur_ctx_set_remap, remap() / undistort(), the host's --undistort): exact
bytes against the numpy restatement of the header's definition (remap_ref.py), which of the two kernels took each launch
against the restated eligibility rule, and, through mi_blur_remap_plan (itself checked against the restated walk in
tests/test_remap_host.py), that the maps reach every branch of the tiled kernel: staged, direct and empty tiles."""
import subprocess

import numpy as np
import pytest

import warp_perspective_ref as pr
import warp_ref as wr
from remap_ref import (BARREL_DIST, BILINEAR, CLAMP, CONSTANT, MAPS, MIXED_OUT, MIXED_SHAPE, NEAREST, affine_map, barrel_K, barrel_map, build_map,
                       make_remap, mixed_map, perspective_map, quantise, ref_plan, ref_remap, takes_tiled)
from resample_harness import (PERSP, REMAP, WARP, apps, blocks, check_gpu_context, check_gpu_context_enlarging, check_pointer_offsets,  # noqa: F401
                              check_synthetic_stream, gpu_run, last, read_ppm, torch_cuda, write_ppm)
from warp_ref import TILED_SHAPES, edge_image

pytestmark = pytest.mark.gpu

TILED, GENERIC = REMAP.tiled, REMAP.generic
BORDERS = (CLAMP, CONSTANT)


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
            got = gpu_run(REMAP, pkg, L, torch_cuda, img, (fmap, BILINEAR, border, 173, 0))
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
            got = gpu_run(REMAP, pkg, L, torch_cuda, img, (fmap, BILINEAR, border, 173, 4096))
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
        got = gpu_run(REMAP, pkg, L, torch_cuda, img, (fmap, BILINEAR, border, 31, 0))
        assert last(L) == TILED and np.array_equal(got, ref_remap(img, fmap, BILINEAR, border, 31)), border


def test_xcd_remap_on_and_off(pkg, L, torch_cuda):
    """One batch with 16 or more workgroups and one with fewer, every channel count."""
    rng = np.random.default_rng(11)
    for c in (1, 2, 3, 4):
        for n, (h, w), (wo, ho) in ((1, (40, 64), (64, 40)), (3, (80, 96), (144, 70))):
            assert (blocks(n, wo, ho, c) >= 16) == (n == 3)
            img = edge_image(rng, n, h, w, c)
            fmap = affine_map(wr.rotation_m(w, h, 33.0, 1.1), wo, ho)
            got = gpu_run(REMAP, pkg, L, torch_cuda, img, (fmap, BILINEAR, CONSTANT, 60, 0))
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
                        got = gpu_run(REMAP, pkg, L, torch_cuda, img, (fmap, BILINEAR, border, 99, 0))
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
                got = gpu_run(REMAP, pkg, L, torch_cuda, img, (fmap, mode, border, 99, 0))
                assert last(L) == GENERIC, (shape, wo, ho, mode)
                assert np.array_equal(got, ref_remap(img, fmap, mode, border, 99)), (shape, name, wo, ho, mode, border)
    # an aligned shape with pointers off 16 bytes, and a map 8 (and 4) bytes off: guards checked inside gpu_run
    img = edge_image(rng, 2, 35, 48, 2)
    check_pointer_offsets(REMAP, pkg, L, torch_cuda, img, (build_map("rot30", 48, 35, 56, 70), BILINEAR, CONSTANT, 5, 0),
                          offsets=((1, 0, 0), (0, 7, 0), (3, 5, 0), (0, 0, 8), (0, 0, 4), (7, 3, 8)))


def test_equivalences_on_the_gpu(pkg, L, torch_cuda):
    """Every affine and perspective warp is a remap: rot30 and keystone maps give the bytes of the warp launches, the x2
    CLAMP map those of the resize."""
    shape, (wo, ho) = TILED_SHAPES[2]
    n, h, w, c = shape
    img = edge_image(np.random.default_rng(21), n, h, w, c)
    m = wr.rotation_m(w, h, 30.0)
    hm = pr.named_maps(w, h, wo, ho)["keystone"]
    for border in BORDERS:
        got = gpu_run(REMAP, pkg, L, torch_cuda, img, (affine_map(m, wo, ho), BILINEAR, border, 40, 0))
        assert last(L) == TILED
        assert np.array_equal(got, gpu_run(WARP, pkg, L, torch_cuda, img, (m, wo, ho, BILINEAR, border, 40))) and last(L) == "blur_warp_tiled_kernel"
        got = gpu_run(REMAP, pkg, L, torch_cuda, img, (perspective_map(hm, wo, ho), BILINEAR, border, 40, 0))
        assert last(L) == TILED
        assert np.array_equal(got, gpu_run(PERSP, pkg, L, torch_cuda, img, (hm, wo, ho, BILINEAR, border, 40))) and last(L) == "blur_warp_persp_tiled_kernel"
    img = np.random.default_rng(9).integers(0, 256, size=(2, 45, 64, 3), dtype=np.uint8)
    got = gpu_run(REMAP, pkg, L, torch_cuda, img, (affine_map(wr.scale_matrix(2, 1), 128, 90), BILINEAR, CLAMP, 0, 0))
    assert last(L) == TILED
    assert np.array_equal(got, pkg.resize(img, (128, 90)))
    assert last(L) == "blur_resize_tiled_kernel"


def test_gpu_equals_cpu_device_on_the_synthetic_stream(pkg, L, torch_cuda):
    fmap = barrel_map(320, 240, 320, 240)
    check_synthetic_stream(REMAP, pkg, L, torch_cuda, [(fmap, mode, CONSTANT, 128, 0) for mode in (BILINEAR, NEAREST)])


@pytest.mark.parametrize("target", [(160, 120), (100, 75)], ids=lambda t: "x".join(map(str, t)))
def test_gpu_context(pkg, L, torch_cuda, target):
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = target
    img = np.random.default_rng(13).integers(0, 256, size=shape, dtype=np.uint8)
    fmap = barrel_map(w, h, wo, ho)
    kernel = TILED if takes_tiled(shape, wo, ho) else GENERIC
    assert (kernel == TILED) == (target == (160, 120))              # 100 x 3 bytes is no whole number of chunks
    check_gpu_context(REMAP, pkg, L, img, (fmap, BILINEAR, CONSTANT, 40, 0), kernel)


def test_gpu_context_enlarging(pkg, L, torch_cuda):
    """160 x 120 to 320 x 240: the output is four times the input, so slots sized by the input would be overrun."""
    shape = (6, 120, 160, 3)
    n, h, w, c = shape
    wo, ho = 320, 240
    img = np.random.default_rng(14).integers(0, 256, size=shape, dtype=np.uint8)
    fmap = barrel_map(w, h, wo, ho)
    check_gpu_context_enlarging(REMAP, pkg, L, img, (fmap, BILINEAR, CONSTANT, 40, 0), fill=40)


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
