"""C-ABI surface and host logic (CPU only): the library loads, exports what include/mi_blur.h
declares, validates arguments, refuses GPU work without a GPU, and its host-side helpers and
CPU device agree with the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest


def test_library_exports_every_declared_symbol(pkg, L):
    decl = pkg.declared_symbols()
    assert len(decl) >= 30
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    missing = [s for s in decl if s not in exported]
    assert not missing, f"declared in include/mi_blur.h but not exported: {missing}"
    assert L.mi_blur_version() == 1


def test_c_header_compiles_as_c(pkg, tmp_path):
    """The boundary is a C ABI: the header must compile as plain C11 and as C++."""
    src = tmp_path / "t.c"
    src.write_text('#include "mi_blur.h"\nint main(void){ mi_blur_timing t; (void)t; return MI_BLUR_OK; }\n')
    inc = os.path.join(pkg.ROOT, "include")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", inc, "-c", str(src),
                    "-o", str(tmp_path / "t.o")], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-x", "c++", "-I", inc, "-c", str(src),
                    "-o", str(tmp_path / "t2.o")], check=True)


def test_product_does_not_link_the_oracle(pkg):
    """The product path must not route through the oracle: no dependency, no symbol."""
    ldd = subprocess.run(["ldd", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle" not in ldd and "ref_blur" not in ldd
    syms = subprocess.run(["nm", "-D", pkg.LIB_PATH], capture_output=True, text=True).stdout
    assert "oracle_" not in syms and "ref_gaussian" not in syms
    # no product source includes, imports or dlopens anything under oracle/
    import re
    for d in (pkg.CSRC, pkg.APPS):
        for f in os.listdir(d):
            if not f.endswith((".cpp", ".hip", ".h")):
                continue
            text = open(os.path.join(d, f)).read()
            assert not re.search(r'#include\s+"[^"]*oracle', text), f
            assert not re.search(r'dlopen\([^)]*oracle', text), f
            assert "liboracle" not in text and "libref_blur" not in text, f
    init = open(os.path.join(pkg.PKG_DIR, "__init__.py")).read()
    assert "import oracle" not in init and "from oracle" not in init and "liboracle" not in init


def test_numa_placement_calls_without_a_gpu(pkg, L):
    """No GPU here: the topology query says so, binding changes nothing, and the placed allocator is plain memory."""
    if L.mi_blur_device_count() > 0:
        pytest.skip("a GPU is visible here")
    assert pkg.device_cpulist(0) == ("", -1)
    buf = C.create_string_buffer(64)
    assert L.mi_blur_device_cpulist(0, buf, len(buf), None) == pkg.ERR_NO_DEVICE
    before = os.sched_getaffinity(0)
    assert L.mi_blur_bind_thread_to_device(0) == 0 and os.sched_getaffinity(0) == before
    p = L.mi_blur_host_alloc_on(0, 4096)
    assert p
    C.memset(p, 7, 4096)
    assert L.mi_blur_host_register(p, 4096) == pkg.OK and L.mi_blur_host_unregister(p) == pkg.OK      # no GPU: nothing to pin
    assert L.mi_blur_host_register(None, 4096) == pkg.ERR_INVALID
    L.mi_blur_host_free(p)


def test_strerror(L):
    assert L.mi_blur_strerror(0) == b"success"
    assert b"invalid" in L.mi_blur_strerror(-1)
    assert b"HIP error" in L.mi_blur_strerror(-1000 - 2)
    assert b"RCCL" in L.mi_blur_strerror(-2000 - 3)


def test_gpu_entry_points_fail_loudly_without_gpu(pkg, L):
    if L.mi_blur_device_count() > 0:
        pytest.skip("a GPU is visible here")
    a = np.zeros(64, np.uint8)
    assert L.mi_blur_enqueue(a.ctypes.data, a.ctypes.data + 32, 2, 2, 3, 1, 1, None) == pkg.ERR_NO_DEVICE
    h = C.c_void_p()
    assert L.mi_blur_create(C.byref(h), 0, 8, 8, 3, 1, 1, 1, 0) == pkg.ERR_NO_DEVICE
    assert not h
    with pytest.raises(pkg.MiBlurError):
        pkg.Context(0, 8, 8, 3)


def test_argument_validation(pkg, L):
    h = C.c_void_p()
    cpu = pkg.DEVICE_CPU
    assert L.mi_blur_create(None, cpu, 8, 8, 3, 1, 1, 1, 0) == pkg.ERR_INVALID
    assert L.mi_blur_create(C.byref(h), cpu, 0, 8, 3, 1, 1, 1, 0) == pkg.ERR_INVALID
    assert L.mi_blur_create(C.byref(h), cpu, 8, 8, 3, 3, 1, 1, 0) == pkg.ERR_INVALID      # radius 3
    assert L.mi_blur_create(C.byref(h), cpu, 8, 8, 3, 1, 0, 1, 0) == pkg.ERR_INVALID      # max_batch 0
    a = np.zeros(8 * 8 * 3, np.uint8)
    b = np.zeros_like(a)
    assert L.mi_blur_cpu_run(a.ctypes.data, a.ctypes.data, 8, 8, 3, 1, 1, 1) == pkg.ERR_INVALID   # in == out
    assert L.mi_blur_cpu_run(a.ctypes.data, b.ctypes.data, 8, 8, 3, 0, 1, 1) == pkg.ERR_INVALID
    assert L.mi_blur_set_option(b"no_such_knob", 1) == pkg.ERR_INVALID
    assert L.mi_blur_set_option(b"rows_per_thread", 12) == pkg.ERR_INVALID
    with pkg.Context(cpu, 8, 8, 3, 1, max_batch=2) as ctx:
        assert L.mi_blur_submit(ctx.h, a.ctypes.data, b.ctypes.data, 3) == pkg.ERR_INVALID  # > max_batch
        assert L.mi_blur_submit(ctx.h, a.ctypes.data, a.ctypes.data, 1) == pkg.ERR_INVALID
        assert L.mi_blur_submit_band(ctx.h, a.ctypes.data, b.ctypes.data, 9, 0, 0) == pkg.ERR_INVALID
        assert L.mi_blur_submit_band(ctx.h, a.ctypes.data, b.ctypes.data, 2, 1, 1) == pkg.ERR_INVALID
        assert L.mi_blur_resident_alloc(ctx.h, 4) == pkg.ERR_STATE                          # CPU device has no HBM pool


def test_set_option_accepts_and_refuses_what_it_did(pkg, L):
    """Every key of mi_blur_set_option with its lowest and highest value, one below and one above, and an unknown key.  The
    expected statuses are literals recorded from the library as it was when every key had its own branch there."""
    OK, INVALID = 0, -1
    assert (pkg.OK, pkg.ERR_INVALID) == (OK, INVALID)
    flags = {"stage_dma": 1, "xcd_remap": 1, "debug_copy": 0, "row_shuffle": 0, "prefer_stream": 0, "zero_copy": 1, "ragged_tiled": 1,
             "fused_release": 0, "experiment": 0, "stream_updown": 1, "debug_xcd_times": 0, "zero_copy_events": 1, "zero_copy_server": 1,
             "staged_server": 1, "zero_copy_trace": 0, "zero_copy_tickets": 1, "zero_copy_spin": 0}          # key: default
    ranges = {"stream_band_rows": (0, 4096, 0), "zero_copy_streams": (1, 8, 4), "zero_copy_blocks": (0, 1 << 20, 24),
              "prefer_direct": (0, 2, 1), "fused_adds_per_word": (4, 4096, 32), "fused_tail_blocks": (10, 800, 25),
              "fused_tail": (0, 500, 30), "fused_window": (1, 4096, 8), "zero_copy_server_min_kb": (0, 1 << 20, 1280),
              "zero_copy_debug_base": (0, 1 << 20, 0), "resident_place_trials": (0, 8, 4), "zero_copy_workers": (1, 2048, 48),
              "zero_copy_idle_us": (10, 100000, 300), "zero_copy_budget": (1, 1 << 20, 256), "xcd_run": (0, 1 << 20, 0)}   # key: lo, hi, default
    lists = {"rows_per_thread": ((0, 4, 8, 16), (-1, 1, 2, 12, 17, 32, 36), 0),
             "direct_bh": ((4, 8, 12, 16), (-1, 0, 3, 5, 17, 32, 36, 40), 8)}                                # key: accepted, refused, default
    assert len(flags) + len(ranges) + len(lists) == 34
    got = []
    try:
        for key in flags:                      # any value is taken (stored as 0 | 1)
            got += [(key, v, L.mi_blur_set_option(key.encode(), v), OK) for v in (0, 1, -1, 2, 2**31 - 1, -2**31)]
        for key, (lo, hi, _) in ranges.items():
            got += [(key, lo, L.mi_blur_set_option(key.encode(), lo), OK), (key, hi, L.mi_blur_set_option(key.encode(), hi), OK),
                    (key, lo - 1, L.mi_blur_set_option(key.encode(), lo - 1), INVALID),
                    (key, hi + 1, L.mi_blur_set_option(key.encode(), hi + 1), INVALID),
                    (key, -2**31, L.mi_blur_set_option(key.encode(), -2**31), INVALID),
                    (key, 2**31 - 1, L.mi_blur_set_option(key.encode(), 2**31 - 1), INVALID)]
        for key, (good, bad, _) in lists.items():
            got += [(key, v, L.mi_blur_set_option(key.encode(), v), OK) for v in good]
            got += [(key, v, L.mi_blur_set_option(key.encode(), v), INVALID) for v in bad + (-2**31, 2**31 - 1)]
        for key in (b"no_such_knob", b"", b"rpg", b"ragged", b"stream_bh", b"stage_dm", b"stage_dma ", b"STAGE_DMA"):   # field names are not keys
            got.append((key.decode(), 1, L.mi_blur_set_option(key, 1), INVALID))
        got.append((None, 1, L.mi_blur_set_option(None, 1), INVALID))
    finally:                                   # back to the built-in defaults
        for key, default in list(flags.items()) + [(k, v[2]) for k, v in list(ranges.items()) + list(lists.items())]:
            assert L.mi_blur_set_option(key.encode(), default) == OK, key
    wrong = [g for g in got if g[2] != g[3]]
    assert not wrong, wrong


def test_a1_partition_matches_reference_formula(pkg, O):
    for mode in (0, 1, 2):
        for bc in (1, 30, 35, 500, 1200):
            for ratio in (0.0, 0.1, 0.5, 0.728, 0.814, 0.837, 1.0):
                assert pkg.a1_partition(mode, bc, ratio) == O.a1_partition(mode, bc, ratio)
    assert pkg.a1_partition(0, 35, 0.728) == (10, 25)          # data/approach1/35_run_1.txt distribution


def test_a2_geometry_matches_reference_formula(pkg, O):
    for h in (3, 16, 240, 256, 1080, 8192):
        for halo in (1, 2):
            for ratio in (0.0, 0.01, 0.163, 0.5, 0.837, 0.99, 1.0):
                assert pkg.a2_split(h, ratio, halo) == O.a2_geometry(h, ratio, halo)
    assert pkg.a2_split(240, 0.837, 1)["split_row"] == 39      # data/approach2/35_run_1.txt:16


def test_shard_range_and_bands_tile_exactly(pkg):
    for n in (1, 7, 5000, 50000):
        for G in (1, 2, 3, 8):
            r = [pkg.shard_range(n, g, G) for g in range(G)]
            assert r[0][0] == 0 and r[-1][1] == n
            assert all(r[i][1] == r[i + 1][0] for i in range(G - 1))
            assert max(e - b for b, e in r) - min(e - b for b, e in r) <= 1
    for H in (16, 240, 1080, 8192):
        for R in (1, 2):
            for G in (1, 2, 5, 8):
                bands = [pkg.band_of(H, R, g, G) for g in range(G)]
                assert bands[0]["row_begin"] == 0 and bands[-1]["row_end"] == H
                assert bands[0]["halo_top"] == 0 and bands[-1]["halo_bottom"] == 0
                for i in range(G - 1):
                    assert bands[i]["row_end"] == bands[i + 1]["row_begin"]
                    assert bands[i]["halo_bottom"] == R and bands[i + 1]["halo_top"] == R


@pytest.mark.parametrize("h,w,c", [(1, 1, 3), (3, 5, 3), (33, 17, 1), (17, 16, 4), (9, 2, 2), (240, 320, 3), (5, 7, 5)])
@pytest.mark.parametrize("radius", [1, 2])
def test_cpu_device_matches_oracle(pkg, L, O, h, w, c, radius):
    """The `cpu` mode device (separable, vectorised) is a different algorithm from the oracle
    (per-pixel 2-D sum): they must agree byte for byte."""
    n = 3
    rng = np.random.default_rng(h + w + c)
    for img in (O.lcg_stream(n, h, w, c), rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)):
        for nt in (1, 4):
            out = np.zeros_like(img)
            pkg.check(L.mi_blur_cpu_run(img.ctypes.data, out.ctypes.data, w, h, c, radius, n, nt))
            want = np.stack([O.blur(np.ascontiguousarray(img[i]), radius) for i in range(n)])
            assert np.array_equal(out, want)


def test_cpu_context_submit_and_band(pkg, L, O):
    h, w, c = 48, 40, 3
    img = O.lcg_stream(6, h, w, c)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=6, n_threads=2) as ctx:
        out = np.zeros_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, 4)
        ctx.submit(img[4:].ctypes.data, out[4:].ctypes.data, 2)
        tm = ctx.sync()
        assert np.array_equal(out, O.blur_batch(img, 1))
        assert tm["images"] == 6 and tm["launches"] == 2 and tm["bytes_alg"] == 2 * img.size
        assert tm["kernel_ms"] > 0 and tm["h2d_ms"] == 0
        assert ctx.timing() == tm                                   # non-blocking snapshot of the same buckets
        assert L.mi_blur_get_timing(ctx.h, None) == pkg.ERR_INVALID
        # Approach 2 on the CPU device: top band [0, split+1) and bottom band [split-1, H)
        one = np.ascontiguousarray(img[0])
        whole = O.blur(one, 1)
        split = 17
        top, bot = np.zeros((split, w, c), np.uint8), np.zeros((h - split, w, c), np.uint8)
        ctx.submit_band(one.ctypes.data, top.ctypes.data, split + 1, 0, 1)
        ctx.submit_band(one[split - 1:].ctypes.data, bot.ctypes.data, h - split + 1, 1, 0)
        ctx.sync()
        assert np.array_equal(np.concatenate([top, bot]), whole)


def test_numpy_convenience_on_the_cpu_device(pkg, O):
    """pkg.blur(): numpy in -> numpy out through create / submit / sync (here on the host-thread device; the GPU form is in
    tests/test_gpu_parity.py): single image, stack, grey image, 3x3 and 5x5, submits in several batches, bad arguments."""
    import numpy as np
    stack = O.lcg_stream(7, 33, 40, 3, first_index=2)
    for ksize in (3, 5):
        want = O.blur_batch(stack, (ksize - 1) // 2)
        assert np.array_equal(pkg.blur(stack, ksize, device=pkg.DEVICE_CPU), want)
        assert np.array_equal(pkg.blur(stack, ksize, device=pkg.DEVICE_CPU, batch=3), want)
        assert np.array_equal(pkg.blur(stack[4], ksize, device=pkg.DEVICE_CPU), want[4])
        grey = np.ascontiguousarray(stack[1][:, :, 0])
        assert np.array_equal(pkg.blur(grey, ksize, device=pkg.DEVICE_CPU)[:, :, 0], O.blur(grey[:, :, None], (ksize - 1) // 2)[:, :, 0])
    assert pkg.blur(np.zeros((0, 8, 8, 3), np.uint8), device=pkg.DEVICE_CPU).shape == (0, 8, 8, 3)
    for bad in (stack.astype(np.float32), np.zeros(5, np.uint8)):
        with pytest.raises(ValueError):
            pkg.blur(bad, device=pkg.DEVICE_CPU)
    with pytest.raises(ValueError):
        pkg.blur(stack, 7, device=pkg.DEVICE_CPU)


def test_synthetic_stream_matches_oracle_generator(pkg, L, O):
    a = np.empty((5, 8, 12, 3), np.uint8)
    L.mi_blur_fill_synthetic(a.ctypes.data, 12, 8, 3, 40, 5, 3)
    assert np.array_equal(a, O.lcg_stream(5, 8, 12, 3, first_index=40))
    assert L.mi_blur_fnv1a64(a.ctypes.data, a.size) == O.fnv1a64(a)


def test_hot_kernels_keep_their_register_budget(pkg, tmp_path):
    """hipcc's schedule of the tile loop is fragile: in round 3 a two-operand v_perm in the x-clamp (needed only for more than
    four channels) made it allocate 39 VGPRs instead of 54 for the 3x3 kernels — loads no longer hoisted — and the headline
    stream lost 20 % without a single test failing.  This compiles the kernels to gfx950 assembly (no GPU needed) and pins
    the VGPR counts of the hot instantiations to the ranges they were tuned in."""
    import re
    out = tmp_path / "k.s"
    r = subprocess.run([pkg.HIPCC, f"--offload-arch={pkg.ARCH}", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(pkg.CSRC, "blur_kernels.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = out.read_text()

    def vgprs(fragment):
        m = re.search(r"\.amdhsa_kernel _ZN7mi_blur\d+" + fragment + r".*?\.end_amdhsa_kernel", text, re.S)
        assert m, fragment
        return int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(0)).group(1))

    budget = {"blur_fused_tail_kernelILi3ELi1ELi8ELb0E": (48, 64),           # the headline kernel (big fused passes): 54
              "blur_fused_kernelILi3ELi1ELi8E": (48, 64),                     # fused passes below 8192 tiles: 54
              "blur_tiled_kernelILi3ELi1ELi8ELb1ELb0ELb0E": (48, 64),          # one-launch 3x3: 54
              "blur_tiled_kernelILi3ELi1ELi4ELb1ELb0ELb0E": (48, 64),          # small grids: 53
              "blur_direct_kernelILi3ELi2ELi8E": (80, 104),                    # 1080p 5x5: 94
              "blur_direct_kernelILi3ELi1ELi8E": (60, 84),                     # small 3x3 launches: 70
              "blur_server_kernelILi3ELi1ELi4ELb0E": (56, 80)}                 # zero-copy batch server: 68
    got = {k: vgprs(k) for k in budget}
    bad = {k: (got[k], budget[k]) for k in budget if not budget[k][0] <= got[k] <= budget[k][1]}
    assert not bad, f"VGPR counts outside the tuned ranges (kernel: (count, (lo, hi))): {bad}"
