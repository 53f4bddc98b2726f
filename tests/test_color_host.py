"""The colour transform (mi_blur_color_preset / _identity / _lut_gamma / _lut_threshold, mi_blur_cpu_run_color,
mi_blur_enqueue_color's argument checks, mi_blur_ctx_set_color, cvt_color() and its kin, the hosts' --color), CPU only:
against the numpy restatement of the header's definition (color_ref.py), independent of the product.  All comparisons
are exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from color_harness import cpu_run, make_color, preset_color
from color_ref import (BIAS_MAX, GROUP, JFIF, MAX_CHANNELS, PRESETS, Q, ROW_MAX, RUN, all_colours, gamma_table, preset, q, random_transform,
                       ref_color, ref_preset, threshold_table)
from filter_harness import MEDIAN, cpu_run as cpu_run_same_size, read_ppm, write_ppm
from resample_harness import check_setters_replace_each_other, needs_gxx, no_scratch, run_sanitized
from resize_ref import ref_resize

PAIRS = [(c, co) for c in range(1, 5) for co in range(1, 5)]


# ---------------------------------------------------------------- presets and table helpers
def test_preset_tables_equal_the_header(pkg, L):
    assert pkg.COLOR_MAX_CHANNELS == MAX_CHANNELS and set(pkg.COLOR_CODES) == set(PRESETS)
    for name, (code, co, shift, rows, bias) in PRESETS.items():
        assert pkg.COLOR_CODES[name] == code
        k = preset_color(pkg, L, name)
        assert (k.out_channels, k.shift, k.lut_on) == (co, shift, 0), name
        want, wbias, _ = preset(name)
        for o in range(4):
            for i in range(4):
                assert k.m[o][i] == (want[o, i] if o < co else 0), (name, o, i)
            assert k.bias[o] == (wbias[o] if o < co else 0), (name, o)
        assert not np.array(k.lut).any()
    # the integers are q() of the JFIF constants; the luma row sums to Q, the chroma rows to 0
    y, cb, cr = PRESETS["rgb2ycbcr"][3]
    assert y == [q(v) for v in JFIF["luma"]] == PRESETS["rgb2gray"][3][0] and sum(y) == Q
    assert cb == [-q(-v) if v < 0 else q(v) for v in JFIF["cb"]] and cr == [-q(-v) if v < 0 else q(v) for v in JFIF["cr"]]
    assert sum(cb) == 0 and sum(cr) == 0
    r, g, b = PRESETS["ycbcr2rgb"][3]
    assert r == [Q, 0, q(JFIF["r"])] and g == [Q, -q(JFIF["g"][0]), -q(JFIF["g"][1])] and b == [Q, q(JFIF["b"]), 0]
    assert PRESETS["bgr2gray"][3][0] == y[::-1]
    k = pkg.Color()
    for bad in (-1, 9, 100):
        assert L.mi_blur_color_preset(bad, C.byref(k)) == pkg.ERR_INVALID
    assert L.mi_blur_color_preset(0, None) == pkg.ERR_INVALID
    with pytest.raises(ValueError):
        pkg.color_preset("rgb2hsv")


def test_properties_over_all_colours(pkg, L):
    """All 2^24 colours through the CPU device: the Y of RGB2YCBCR is RGB2GRAY, the round trip stays within 1, and both
    directions equal the restatement."""
    img = all_colours()
    ycc = cpu_run(pkg, L, img, preset_color(pkg, L, "rgb2ycbcr"), 0)
    assert np.array_equal(ycc, ref_preset(img, "rgb2ycbcr"))
    gray = cpu_run(pkg, L, img, preset_color(pkg, L, "rgb2gray"), 0)
    assert np.array_equal(gray[..., 0], ycc[..., 0])
    back = cpu_run(pkg, L, ycc, preset_color(pkg, L, "ycbcr2rgb"), 0)
    assert np.array_equal(back, ref_preset(ycc, "ycbcr2rgb"))
    assert np.abs(back.astype(np.int16) - img.astype(np.int16)).max() <= 1
    # the clamp is live in the forward direction: pure blue gives Cb = 256 before it
    m, bias, shift = preset("rgb2ycbcr")
    assert (int(m[1, 2]) * 255 + int(bias[1])) >> shift == 256
    assert tuple(ycc[0, 0, 255]) == (29, 255, 107)                      # colour (0, 0, 255) is pixel 255


def test_greys_stay_grey(pkg, L):
    v = np.arange(256, dtype=np.uint8)
    grey = np.stack([v, v, v], axis=-1).reshape(1, 16, 16, 3)
    assert np.array_equal(cpu_run(pkg, L, grey, preset_color(pkg, L, "rgb2gray"), 1)[..., 0], grey[..., 0])
    assert np.array_equal(cpu_run(pkg, L, grey, preset_color(pkg, L, "bgr2gray"), 1)[..., 0], grey[..., 0])
    ycc = cpu_run(pkg, L, grey, preset_color(pkg, L, "rgb2ycbcr"), 1)
    assert np.array_equal(ycc[..., 0], grey[..., 0]) and (ycc[..., 1:] == 128).all()
    assert np.array_equal(cpu_run(pkg, L, ycc, preset_color(pkg, L, "ycbcr2rgb"), 1), grey)
    one = np.ascontiguousarray(grey[..., :1])
    assert np.array_equal(cpu_run(pkg, L, one, preset_color(pkg, L, "gray2rgb"), 1), grey)


def test_permutations_and_alpha(pkg, L):
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, size=(2, 9, 11, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, size=(2, 9, 11, 4), dtype=np.uint8)
    bgr = cpu_run(pkg, L, rgb, preset_color(pkg, L, "rgb2bgr"), 2)
    assert np.array_equal(bgr, rgb[..., ::-1])
    assert np.array_equal(cpu_run(pkg, L, bgr, preset_color(pkg, L, "rgb2bgr"), 2), rgb)            # twice: the identity
    assert np.array_equal(cpu_run(pkg, L, rgba, preset_color(pkg, L, "rgba2bgra"), 2), rgba[..., [2, 1, 0, 3]])
    with_alpha = cpu_run(pkg, L, rgb, preset_color(pkg, L, "rgb2rgba"), 2)
    assert (with_alpha[..., 3] == 255).all() and np.array_equal(with_alpha[..., :3], rgb)
    assert np.array_equal(cpu_run(pkg, L, with_alpha, preset_color(pkg, L, "rgba2rgb"), 2), rgb)
    # the presets do not fix C: RGB2GRAY on four channels ignores alpha
    assert np.array_equal(cpu_run(pkg, L, rgba, preset_color(pkg, L, "rgb2gray"), 2), ref_preset(rgba[..., :3], "rgb2gray"))
    for c in range(1, 5):
        k = pkg.Color()
        assert L.mi_blur_color_identity(c, C.byref(k)) == pkg.OK and (k.out_channels, k.shift, k.lut_on) == (c, 0, 0)
        img = rng.integers(0, 256, size=(1, 5, 7, c), dtype=np.uint8)
        assert np.array_equal(cpu_run(pkg, L, img, k, 1), img)
    for bad in (0, 5, -1):
        assert L.mi_blur_color_identity(bad, C.byref(pkg.Color())) == pkg.ERR_INVALID
    assert L.mi_blur_color_identity(3, None) == pkg.ERR_INVALID


def test_lut_helpers(pkg, L):
    t = (C.c_uint8 * 256)()
    assert L.mi_blur_color_lut_gamma(1.0, t) == pkg.OK and list(t) == list(range(256))
    for g in (0.45, 2.2, 5.0):
        assert L.mi_blur_color_lut_gamma(g, t) == pkg.OK and np.array_equal(np.array(t), gamma_table(g)), g
        assert t[0] == 0 and t[255] == 255
    for g in (0.0, -1.0, float("inf"), float("nan")):
        assert L.mi_blur_color_lut_gamma(g, t) == pkg.ERR_INVALID
    assert L.mi_blur_color_lut_gamma(2.0, None) == pkg.ERR_INVALID
    assert L.mi_blur_color_lut_threshold(-1, 3, 200, t) == pkg.OK and set(t) == {200}
    assert L.mi_blur_color_lut_threshold(255, 3, 200, t) == pkg.OK and set(t) == {3}
    assert L.mi_blur_color_lut_threshold(100, 0, 255, t) == pkg.OK and np.array_equal(np.array(t), threshold_table(100))
    assert t[100] == 0 and t[101] == 255
    for bad in ((-2, 0, 255), (256, 0, 255), (5, -1, 255), (5, 0, 256), (5, 256, 0)):
        assert L.mi_blur_color_lut_threshold(*bad, t) == pkg.ERR_INVALID, bad
    assert L.mi_blur_color_lut_threshold(5, 0, 255, None) == pkg.ERR_INVALID


# ---------------------------------------------------------------- the CPU device against the restatement
@pytest.mark.parametrize("lut_on", [0, 1])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_cpu_run_matches_the_restatement(pkg, L, pair, lut_on):
    """Signed weights at the row-sum limit with a bias of +-2^26, and spread ones, at shift 0 and 16; 1, 3 and 7 threads."""
    c, co = pair
    rng = np.random.default_rng(100 * c + 10 * co + lut_on)
    img = rng.integers(0, 256, size=(3, 19, 23, c), dtype=np.uint8)
    img[0, :4] = 0
    img[0, 4:8] = 255
    for shift in (0, 16):
        for limit in (True, False):
            m, bias, _, lut = random_transform(rng, c, co, lut_on, shift, limit)
            k = make_color(pkg, m, bias, shift, lut)
            want = ref_color(img, m, bias, shift, lut)
            assert want.shape == (3, 19, 23, co)
            for nt in (1, 3, 7):
                assert np.array_equal(cpu_run(pkg, L, img, k, nt), want), (pair, lut_on, shift, limit, nt)


def test_lut_off_ignores_a_garbage_table(pkg, L):
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(1, 6, 7, 3), dtype=np.uint8)
    m, bias, shift = preset("rgb2ycbcr")
    junk = rng.integers(0, 256, size=(3, 256), dtype=np.uint8)
    assert np.array_equal(cpu_run(pkg, L, img, make_color(pkg, m, bias, shift, junk, lut_on=0), 1), ref_color(img, m, bias, shift))


# ---------------------------------------------------------------- statuses
def bad_colors(pkg):
    """Color structs the header calls invalid, each one field away from a good one."""
    def one(**kw):
        m, bias, shift = preset("rgb2ycbcr")
        k = make_color(pkg, m, bias, shift)
        for name, v in kw.items():
            if name == "row":
                k.m[1][0], k.m[1][1], k.m[1][2], k.m[1][3] = v
            elif name == "bias1":
                k.bias[1] = v
            else:
                setattr(k, name, v)
        return k
    return [one(out_channels=0), one(out_channels=5), one(out_channels=-1), one(shift=-1), one(shift=17), one(lut_on=2), one(lut_on=-1),
            one(row=(ROW_MAX, 0, -1, 0)), one(row=(0, 0, 0, ROW_MAX + 1)), one(row=(-ROW_MAX, 0, 0, 1)),     # a column beyond C counts
            one(bias1=BIAS_MAX + 1), one(bias1=-BIAS_MAX - 1)]


def good_at_the_limits(pkg):
    k = make_color(pkg, *preset("rgb2ycbcr"))
    k.m[1][0], k.m[1][1], k.m[1][2], k.m[1][3] = ROW_MAX - 2, -1, 0, 1
    k.bias[1], k.bias[2] = BIAS_MAX, -BIAS_MAX
    C.memset(C.byref(k, type(k).m.offset + 3 * 16), 0x7F, 16)          # row 3, beyond out_channels: garbage is accepted
    k.bias[3] = -2**31
    return k


def calls(pkg, L, call):
    """call(in, out, w, h, c, n, k) -> status over everything the header calls invalid; returns the good buffers."""
    a, b = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 4), np.uint8)
    ia, ib = a.ctypes.data, b.ctypes.data
    good = C.byref(good_at_the_limits(pkg))
    for k in bad_colors(pkg):
        assert call(ia, ib, 8, 8, 3, 1, C.byref(k)) == pkg.ERR_INVALID
    for args in [(ia, ib, 8, 8, 3, 1, None), (None, ib, 8, 8, 3, 1, good), (ia, None, 8, 8, 3, 1, good), (ia, ia, 8, 8, 3, 1, good),
                 (ia, ib, 8, 8, 5, 1, good), (ia, ib, 8, 8, 0, 1, good), (ia, ib, 0, 8, 3, 1, good), (ia, ib, 8, 0, 3, 1, good), (ia, ib, -1, 8, 3, 1, good),
                 (ia, ib, 32769, 1, 1, 1, good), (ia, ib, 1, 32769, 1, 1, good), (ia, ib, 8, 8, 3, -1, good)]:
        assert call(*args) == pkg.ERR_INVALID, args[2:6]
    # the image's byte limits hold for the output too: 32768 x 32768 x 1 is 1 GiB in, 3 GiB out
    assert call(ia, ib, 32768, 32768, 1, 1, C.byref(preset_color(pkg, L, "gray2rgb"))) == pkg.ERR_INVALID
    return ia, ib, good


def test_cpu_run_refuses_invalid_arguments(pkg, L):
    ia, ib, good = calls(pkg, L, lambda i, o, w, h, c, n, k: L.mi_blur_cpu_run_color(i, o, w, h, c, n, k, 1))
    assert L.mi_blur_cpu_run_color(ia, ib, 8, 8, 3, 1, good, 1) == pkg.OK
    assert L.mi_blur_cpu_run_color(ia, ib, 8, 8, 3, 0, good, 1) == pkg.OK


def test_enqueue_invalid_comes_before_no_device(pkg, L):
    ia, ib, good = calls(pkg, L, lambda i, o, w, h, c, n, k: L.mi_blur_enqueue_color(i, o, w, h, c, n, k, None))
    if L.mi_blur_device_count() <= 0:
        assert L.mi_blur_enqueue_color(ia, ib, 8, 8, 3, 1, good, None) == pkg.ERR_NO_DEVICE
        assert L.mi_blur_enqueue_color(ia, ib, 8, 8, 3, 0, good, None) == pkg.ERR_NO_DEVICE
    else:
        assert L.mi_blur_enqueue_color(ia, ib, 8, 8, 3, 0, good, None) == pkg.OK


def test_ctx_set_refuses_invalid_arguments(pkg, L):
    good = good_at_the_limits(pkg)
    with pkg.Context(pkg.DEVICE_CPU, 8, 8, 3, 1, max_batch=1) as ctx:
        assert L.mi_blur_ctx_set_color(None, C.byref(good)) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_color(ctx.h, None) == pkg.ERR_INVALID
        for k in bad_colors(pkg):
            assert L.mi_blur_ctx_set_color(ctx.h, C.byref(k)) == pkg.ERR_INVALID
        assert L.mi_blur_ctx_set_color(ctx.h, C.byref(good)) == pkg.OK
    with pkg.Context(pkg.DEVICE_CPU, 8, 8, 5, 1, max_batch=1) as five:                  # C > 4, checked where C is known
        assert L.mi_blur_ctx_set_color(five.h, C.byref(good)) == pkg.ERR_INVALID


# ---------------------------------------------------------------- CPU-device contexts
@pytest.mark.parametrize("name", ["rgb2gray", "rgb2bgr", "rgb2rgba"])               # Co < C, Co = C, Co > C
def test_cpu_context(pkg, L, name):
    """The setter's struct is overwritten after the call: the context keeps a copy.  Co > C writes more than it reads."""
    rng = np.random.default_rng(23)
    img = rng.integers(0, 256, size=(5, 37, 42, 3), dtype=np.uint8)
    n, h, w, c = img.shape
    want = ref_preset(img, name)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n, n_threads=3) as ctx:
        k = preset_color(pkg, L, name)
        assert L.mi_blur_ctx_set_color(ctx.h, C.byref(k)) == pkg.OK
        C.memset(C.byref(k), 0xFF, C.sizeof(k))
        out = np.full(want.size + 128, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data + 64, n)
        t = ctx.sync()
        assert np.array_equal(out[64:64 + want.size].reshape(want.shape), want)
        assert (out[:64] == 0xA5).all() and (out[64 + want.size:] == 0xA5).all()
        assert t["bytes_alg"] == n * w * h * (c + want.shape[-1]) and t["images"] == n
        o = np.zeros((n, h, w, 4), np.uint8)
        assert L.mi_blur_submit_band(ctx.h, img.ctypes.data, o.ctypes.data, 20, 2, 2) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_submit_bands(ctx.h, img.ctypes.data, o.ctypes.data, n, h * w * c, 20, 2, 2) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_submit_planar(ctx.h, img.ctypes.data, o.ctypes.data, n, 0) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_resident_run(ctx.h, 1, 1, 0) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_resident_run_fused(ctx.h, 1, 1, 0) == pkg.ERR_UNSUPPORTED
        assert not o.any()
        assert L.mi_blur_ctx_set_color(ctx.h, C.byref(preset_color(pkg, L, name))) == pkg.ERR_STATE


def test_setters_replace_each_other(pkg, L):
    rng = np.random.default_rng(29)
    img = rng.integers(0, 256, size=(2, 20, 24, 3), dtype=np.uint8)
    gray = lambda ctx: ctx.set_color(pkg.color_preset("rgb2gray"))
    rgba = lambda ctx: ctx.set_color(pkg.color_preset("rgb2rgba"))
    resize = lambda ctx: ctx.set_resize(40, 31)
    median = lambda ctx: ctx.set_median(1)
    med = cpu_run_same_size(MEDIAN, pkg, L, img, 1, 1)
    check_setters_replace_each_other(pkg, L, img, [([gray, resize], ref_resize(img, 40, 31)), ([resize, gray], ref_preset(img, "rgb2gray")),
                                                   ([gray, median], med), ([median, rgba], ref_preset(img, "rgb2rgba")),
                                                   ([rgba, gray], ref_preset(img, "rgb2gray")), ([gray, rgba], ref_preset(img, "rgb2rgba"))])


# ---------------------------------------------------------------- Python
def test_numpy_functions_on_the_cpu_device(pkg, L):
    rng = np.random.default_rng(31)
    cpu = pkg.DEVICE_CPU
    stacks = {c: rng.integers(0, 256, size=(4, 15, 21, c), dtype=np.uint8) for c in (1, 3, 4)}
    for name, (code, co, shift, rows, bias) in PRESETS.items():
        stack = stacks[len(rows[0])]
        want = ref_preset(stack, name)
        got = pkg.cvt_color(stack, name, device=cpu, batch=3)
        assert got.dtype == np.uint8 and got.shape == (4, 15, 21, co) and np.array_equal(got, want), name
        if len(rows[0]) == 1:
            one = pkg.cvt_color(stack[0, :, :, 0], name, device=cpu)     # a 2-D array is one grey image
            assert one.shape == (15, 21, co) and np.array_equal(one, want[0])
        else:
            one = pkg.cvt_color(stack[0], name, device=cpu)
            assert one.shape == ((15, 21) if co == 1 else (15, 21, co)) and np.array_equal(one.reshape(want[0].shape), want[0]), name
    rgb, grey = stacks[3], stacks[1][0, :, :, 0]
    assert np.array_equal(pkg.threshold(rgb, 100, device=cpu), np.where(rgb > 100, 255, 0))
    assert np.array_equal(pkg.threshold(grey, 7, 10, 20, device=cpu), np.where(grey > 7, 20, 10))
    assert pkg.threshold(grey, 7, device=cpu).shape == grey.shape
    assert np.array_equal(pkg.gamma_correct(rgb, 2.2, device=cpu), gamma_table(2.2)[rgb])
    inv = np.arange(255, -1, -1)
    assert np.array_equal(pkg.apply_lut(rgb, inv, device=cpu), 255 - rgb)
    per = np.stack([rng.permutation(256) for _ in range(3)])
    assert np.array_equal(pkg.apply_lut(rgb, per, device=cpu), np.stack([per[o][rgb[..., o]] for o in range(3)], axis=-1))
    m, bias, shift, lut = random_transform(rng, 3, 2, 1, 16, False)
    got = pkg.color_transform(rgb, m[:, :3], bias, shift, lut, device=cpu, batch=2)
    assert got.shape == (4, 15, 21, 2) and np.array_equal(got, ref_color(rgb, m, bias, shift, lut))
    assert np.array_equal(pkg.color_transform(rgb[0], [[0, 1, 0]], device=cpu), rgb[0, :, :, 1])
    empty = pkg.cvt_color(np.zeros((0, 15, 21, 3), np.uint8), "rgb2rgba", device=cpu)
    assert empty.shape == (0, 15, 21, 4) and empty.dtype == np.uint8
    for bad in (lambda: pkg.cvt_color(rgb, "rgb2hsv", device=cpu), lambda: pkg.cvt_color(rgb.astype(np.float32), "rgb2gray", device=cpu),
                lambda: pkg.color_transform(rgb, [[1, 1]], device=cpu), lambda: pkg.apply_lut(rgb, np.arange(255), device=cpu),
                lambda: pkg.cvt_color(np.zeros((2, 4, 4, 5), np.uint8), "rgb2gray", device=cpu)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(pkg.MiBlurError):
        pkg.color_transform(rgb, [[ROW_MAX, 1, 0]], device=cpu)
    with pytest.raises(pkg.MiBlurError):
        pkg.gamma_correct(rgb, 0.0, device=cpu)


# ---------------------------------------------------------------- hosts
def test_hosts_color_flags(pkg, tmp_path):
    pkg.build_native()
    het, split = (os.path.join(pkg.APPS, a) for a in ("heterogeneous_blur", "split_image_blur"))
    img = np.random.default_rng(19).integers(0, 256, size=(24, 32, 3), dtype=np.uint8)
    src = tmp_path / "in.ppm"
    write_ppm(src, img)
    base = [het, "cpu", "0", "35", "--image", str(src), "--images", "4"]
    run = lambda *a: subprocess.run([*base, *a], capture_output=True, text=True, timeout=60)
    for other in (["--median", "3"], ["--resize", "16x12"], ["--ksize", "5"], ["--sigma", "1.5"], ["--conv", "sobel"], ["--pyr-down"], ["--rotate", "10"]):
        r = run("--color", "gray", *other)
        assert r.returncode != 0 and "Error: --color, --gamma and --threshold exclude" in r.stdout, other
    r = run("--threshold", "100", "--median", "3")
    assert r.returncode != 0 and "Error: --color, --gamma and --threshold exclude" in r.stdout
    r = run("--color", "hsv")
    assert r.returncode != 0 and "Error: --color gray|bgr|ycbcr|from-ycbcr" in r.stdout
    r = run("--gamma", "2", "--threshold", "3")
    assert r.returncode != 0 and "Error: --gamma excludes --threshold" in r.stdout
    r = run("--color", "gray", "--resident")
    assert r.returncode != 0 and "exclude --resident and --frames" in r.stdout
    r = subprocess.run([split, "0.5", "35", "--image", str(src), "--images", "4", "--color", "gray"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--color" in r.stdout and "bands are not supported" in r.stdout

    dst = tmp_path / "out.pgm"
    r = run("--color", "gray", "--save", str(dst))
    assert r.returncode == 0 and "Blur kernel: colour transform gray, 3 -> 1 channels" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert dst.read_bytes() == b"P5\n32 24\n255\n" + ref_preset(img[None], "rgb2gray").tobytes()
    cases = [(("--color", "ycbcr"), "ycbcr", ref_preset(img[None], "rgb2ycbcr")), (("--color", "bgr"), "bgr", img[None, ..., ::-1]),
             (("--color", "from-ycbcr", "--gamma", "2.2"), "from-ycbcr+gamma", gamma_table(2.2)[ref_preset(img[None], "ycbcr2rgb")]),
             (("--threshold", "128"), "threshold", threshold_table(128)[img[None]]), (("--gamma", "0.5"), "gamma", gamma_table(0.5)[img[None]])]
    for flags, name, want in cases:
        dst = tmp_path / f"{name}.ppm"
        r = run(*flags, "--save", str(dst))
        assert r.returncode == 0 and f"Blur kernel: colour transform {name}, 3 -> 3 channels" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        assert np.array_equal(read_ppm(dst), want[0]), name


# ---------------------------------------------------------------- the kernels' code, the CPU device under sanitizers
def test_tiled_kernels_use_no_scratch(pkg, tmp_path):
    """Compiles color_kernels.hip to gfx950 assembly (no GPU needed): 16 (C, Co) pairs x lut_on, and a pointwise kernel
    must not spill or index registers at run time."""
    no_scratch(pkg, tmp_path, "color_kernels.hip", "blur_color_tiled_kernel", 32)
    assert (GROUP, RUN) == (16, 256)
    text = open(os.path.join(pkg.CSRC, "filter.h")).read()
    assert "constexpr int COLOR_GROUP = 16;" in text and "constexpr int COLOR_RUN = 256;" in text     # color_ref.py's copies


@needs_gxx
def test_color_clean_under_asan_ubsan(pkg, tmp_path):
    run_sanitized(pkg, tmp_path, ("san_color.cpp", "cpu_device.cpp"), ["tile geometry clean", "random color cases clean", "limit color cases clean"])
