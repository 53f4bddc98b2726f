"""What the test files of the five filters whose output size differs from the input's share
(tests/test_{sep_down,resize,warp,warp_perspective,remap}_{gpu,host}.py; not a test module, and not a conftest: fixtures reach
a test file by plain import into its namespace).  It is filter_harness.py for these five: that one's Family assumes an
output of the input's size and a band form, which these do not have.

A Resampler holds what the families differ in: the kernel names, the structs their exports take, the output size, the
Context setter, the numpy restatement and the eligibility rule of the tiled kernel.  A spec is the family's filter value:
    sep_down                  (SepKernel, (sx, sy, ox, oy))
    resize                    (wo, ho, mode)
    warp, warp_perspective    (m, wo, ho, mode, border, fill)         m: the 6 (affine) or 9 (homography) integers
    remap                     (fmap, mode, border, fill, stage_bytes)  fmap: int32 (Ho, Wo, 2), always the spec's first entry
gpu_run / cpu_run launch one spec through the C ABI inside guard bytes; the check_* functions are the bodies the family
files had in common.  They take the family, the image, the spec and every number the copies differed in; the loops over
shapes, maps, modes and borders, the seeds and the parametrize lists stay in the family files."""
import contextlib
import ctypes as C
import os
import re
import shutil
import subprocess
import typing

import numpy as np
import pytest

import remap_ref
import resize_ref
import warp_perspective_ref
import warp_ref
from filter_harness import apps, read_ppm, torch_cuda, write_ppm  # noqa: F401  (re-exported to the family files)
from sep_down_ref import down_shape, ref_sep_down

MAX_DIM = resize_ref.MAX_DIM


# ---------------------------------------------------------------- the families
class Resampler(typing.NamedTuple):
    name: str                       # of mi_blur_enqueue_<name>, mi_blur_cpu_run_<name> and mi_blur_ctx_set_<name>
    tiled: str                      # the kernel of the launches takes_tiled() admits ...
    generic: str                    # ... and of every other launch
    structs: typing.Callable        # (pkg, spec) -> the structs the three exports take by reference, in their order
    out_size: typing.Callable       # (spec, w, h) -> (wo, ho)
    set: typing.Callable            # (Context, pkg, spec): Context.set_*, which raises on a status
    ref: typing.Callable            # (img N x H x W x C, spec) -> the numpy restatement, N x Ho x Wo x C
    takes_tiled: typing.Callable    # (shape, spec, offset_in=0, offset_out=0[, offset_map=0]) -> the header's rule for the tiled kernel
    fmap: typing.Callable = lambda spec: None     # remap alone: the spec's map, whose address the exports take after the struct

    def args(self, pkg, spec, map_ptr=None, structs=None):
        """What the exports take between n_images (the context, for ctx_set) and the stream or thread count: the structs
        (fresh ones unless given) by reference, then remap's map."""
        a = tuple(C.byref(s) for s in structs or self.structs(pkg, spec))
        return a if self.fmap(spec) is None else a + (map_ptr,)

    def enqueue(self, L, d_in, d_out, w, h, c, n, args, stream):
        return getattr(L, f"mi_blur_enqueue_{self.name}")(d_in, d_out, w, h, c, n, *args, stream)

    def cpu_run(self, L, i, o, w, h, c, n, args, n_threads):
        return getattr(L, f"mi_blur_cpu_run_{self.name}")(i, o, w, h, c, n, *args, n_threads)

    def ctx_set(self, L, ctx, args):
        return getattr(L, f"mi_blur_ctx_set_{self.name}")(ctx, *args)

    def host_args(self, pkg, spec, structs=None):
        """args() with the map, if any, in host memory (the spec keeps it alive): for cpu_run and ctx_set."""
        m = self.fmap(spec)
        return self.args(pkg, spec, None if m is None else m.ctypes.data, structs)

    def kernel(self, shape, spec, *offsets):
        return self.tiled if self.takes_tiled(shape, spec, *offsets) else self.generic


def _down_takes_tiled(shape, spec, offset_in=0, offset_out=0):
    """The header's rule for blur_sep_down_tiled_kernel: stride 2 x 2, 1-4 channels, rows of a multiple of 32 bytes (dense
    images are then whole chunks apart, in and out), both pointers aligned."""
    (n, h, w, c), (sx, sy, _, _) = shape, spec[1]
    return sx == sy == 2 and 1 <= c <= 4 and (w * c) % 32 == 0 and offset_in % 16 == 0 and offset_out % 16 == 0


def _down_size(spec, w, h):
    n, ho, wo, c = down_shape((1, h, w, 1), *spec[1])
    return wo, ho


def _warp_family(name, kernels, make, ref):
    """The affine and the perspective warp: one struct that holds the output size and the integers of the map."""
    return Resampler(
        name, f"blur_{kernels}_tiled_kernel", f"blur_{kernels}_generic_kernel",
        structs=lambda pkg, s: (make(pkg, *s),),
        out_size=lambda s, w, h: (s[1], s[2]),
        set=lambda ctx, pkg, s: getattr(ctx, f"set_{name}")(make(pkg, *s)),
        ref=lambda img, s: ref.ref_warp(img, *s),
        takes_tiled=lambda shape, s, oi=0, oo=0: ref.takes_tiled(shape, *s[:5], oi, oo))


SEP_DOWN = Resampler(
    "sep_down", "blur_sep_down_tiled_kernel", "blur_sep_down_generic_kernel",
    structs=lambda pkg, s: (s[0], pkg.Decimation(*s[1])),
    out_size=_down_size,
    set=lambda ctx, pkg, s: ctx.set_sep_down(s[0], *s[1]),
    ref=lambda img, s: ref_sep_down(img, *s[0].taps(), *s[1]),
    takes_tiled=_down_takes_tiled)
RESIZE = Resampler(
    "resize", "blur_resize_tiled_kernel", "blur_resize_generic_kernel",
    structs=lambda pkg, s: (pkg.Resize(*s),),
    out_size=lambda s, w, h: (s[0], s[1]),
    set=lambda ctx, pkg, s: ctx.set_resize(*s),
    ref=lambda img, s: resize_ref.ref_resize(img, *s),
    takes_tiled=lambda shape, s, oi=0, oo=0: resize_ref.takes_tiled(shape, *s, oi, oo))
WARP = _warp_family("warp", "warp", warp_ref.make_warp, warp_ref)
PERSP = _warp_family("warp_perspective", "warp_persp", warp_perspective_ref.make_persp, warp_perspective_ref)
REMAP = Resampler(
    "remap", "blur_remap_tiled_kernel", "blur_remap_generic_kernel",
    structs=lambda pkg, s: (remap_ref.make_remap(pkg, s[0].shape[1], s[0].shape[0], *s[1:]),),
    out_size=lambda s, w, h: (s[0].shape[1], s[0].shape[0]),
    set=lambda ctx, pkg, s: ctx.set_remap(remap_ref.make_remap(pkg, s[0].shape[1], s[0].shape[0], *s[1:]), s[0]),
    ref=lambda img, s: remap_ref.ref_remap(img, *s[:4]),
    takes_tiled=lambda shape, s, oi=0, oo=0, om=0: remap_ref.takes_tiled(shape, s[0].shape[1], s[0].shape[0], s[1], oi, oo, om),
    fmap=lambda s: s[0])


# ---------------------------------------------------------------- small helpers
def last(L):
    return L.mi_blur_last_kernel().decode()


def blocks(n, wo, ho, c):
    """Workgroups of a tiled launch of the warp, perspective or remap kernel (warp_ref.tile_geometry: theirs alike)."""
    ncols, cpr, rows = warp_ref.tile_geometry(wo, ho, c)
    return n * -(-cpr // ncols) * -(-ho // rows)


def spans_tiles(wo, ho, c, tile_geometry=warp_ref.tile_geometry):
    """More than one tile both ways."""
    ncols, cpr, rows = tile_geometry(wo, ho, c)
    return cpr > ncols and ho > rows


@contextlib.contextmanager
def pinned(L, *sizes):
    """Pinned host buffers of `sizes` bytes: [(address, uint8 array over it)], freed on the way out."""
    ptrs = [L.mi_blur_host_alloc(s) for s in sizes]
    try:
        yield [(p, np.ctypeslib.as_array((C.c_uint8 * s).from_address(p))) for p, s in zip(ptrs, sizes)]
    finally:
        for p in ptrs:
            L.mi_blur_host_free(p)


def no_scratch(pkg, tmp_path, source, kernel_pattern, count, dynamic_lds_only=False):
    """Compiles csrc/<source> to gfx950 assembly (no GPU needed): there are `count` kernels whose name holds kernel_pattern,
    and none of them spills or indexes registers at run time.  dynamic_lds_only: nor has one a static LDS segment (the warp
    and remap kernels size all their LDS per launch; the sep_down and resize kernels declare theirs)."""
    out = tmp_path / "k.s"
    r = subprocess.run([pkg.HIPCC, f"--offload-arch={pkg.ARCH}", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", str(out),
                        os.path.join(pkg.CSRC, source)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"\.amdhsa_kernel (\S*%s\S*)(.*?)\.end_amdhsa_kernel" % kernel_pattern, out.read_text(), re.S)
    assert len(kernels) == count, [k for k, _ in kernels]
    for name, body in kernels:
        assert re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1) == "0", name
        if dynamic_lds_only:
            assert re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1) == "0", name


needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def run_sanitized(pkg, tmp_path, sources, expect, argv=()):
    """Builds tests/<sources[0]> (a program with its own main) and csrc/<the others> with g++ under ASan and UBSan, runs it
    with argv, and wants exit status 0, every string of `expect` and no "FAILED" on stdout, and no report on stderr."""
    root = os.path.dirname(os.path.abspath(__file__))
    exe = tmp_path / os.path.splitext(sources[0])[0]
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I", pkg.CSRC, os.path.join(root, sources[0])]
    if sources[1:]:                                                  # the CPU device starts threads
        cmd += [os.path.join(pkg.CSRC, s) for s in sources[1:]] + ["-lpthread"]
    subprocess.run(cmd + ["-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe), *map(str, argv)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and all(e in r.stdout for e in expect) and "FAILED" not in r.stdout, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


# ---------------------------------------------------------------- one launch
def gpu_run(fam, pkg, L, torch, host, spec, offset_in=0, offset_out=0, offset_map=0):
    """host: N x H x W x C -> mi_blur_enqueue_*.  The input lies offset_in bytes into a buffer with 64 spare bytes, the
    output offset_out bytes into one with 128 bytes of 0x5A to spare: guards either side.  Remap's map lies offset_map
    bytes (a multiple of 4) into a buffer with 64 spare bytes."""
    n, h, w, c = host.shape
    wo, ho = fam.out_size(spec, w, h)
    size_out = n * ho * wo * c
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    map_ptr = None
    if fam.fmap(spec) is not None:
        mbytes = np.ascontiguousarray(fam.fmap(spec), dtype=np.int32).view(np.uint8).reshape(-1)
        d_map = torch.zeros(mbytes.size + 64, dtype=torch.uint8, device="cuda")
        d_map[offset_map:offset_map + mbytes.size] = torch.from_numpy(mbytes).cuda()
        assert d_map.data_ptr() % 16 == 0
        map_ptr = d_map.data_ptr() + offset_map
    rc = fam.enqueue(L, d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, fam.args(pkg, spec, map_ptr),
                     torch.cuda.current_stream().cuda_stream)
    pkg.check(rc, f"mi_blur_enqueue_{fam.name}")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, ho, wo, c)


def cpu_run(fam, pkg, L, img, spec, n_threads, guard=256):
    """img: N x H x W x C -> mi_blur_cpu_run_*.  The output starts as 0xA5, so a byte left unwritten shows (the callers'
    images and fills avoid giving 0xA5 everywhere), and the `guard` bytes before and after it must still hold 0xA5."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    wo, ho = fam.out_size(spec, w, h)
    size_out = n * ho * wo * c
    buf = np.full(size_out + 2 * guard, 0xA5, np.uint8)
    pkg.check(fam.cpu_run(L, a.ctypes.data, buf.ctypes.data + guard, w, h, c, n, fam.host_args(pkg, spec), n_threads), f"mi_blur_cpu_run_{fam.name}")
    assert (buf[:guard] == 0xA5).all() and (buf[guard + size_out:] == 0xA5).all(), "wrote outside the output"
    return buf[guard:guard + size_out].reshape(n, ho, wo, c)


# ---------------------------------------------------------------- shared bodies: the GPU
def check_pointer_offsets(fam, pkg, L, torch, img, spec, offsets=((1, 0), (0, 7), (3, 5))):
    """An aligned shape takes the tiled kernel; with a pointer off 16 bytes (`offsets`: input, output[, map]) it takes the
    generic kernel and gives the same bytes, the guards inside gpu_run intact."""
    want = fam.ref(img, spec)
    assert fam.takes_tiled(img.shape, spec)
    assert np.array_equal(gpu_run(fam, pkg, L, torch, img, spec), want) and last(L) == fam.tiled
    for off in offsets:
        assert not fam.takes_tiled(img.shape, spec, *off)
        assert np.array_equal(gpu_run(fam, pkg, L, torch, img, spec, *off), want), off
        assert last(L) == fam.generic, off


def check_synthetic_stream(fam, pkg, L, torch, specs, shape=(4, 240, 320, 3), n_threads=4):
    """The CPU device equals the restatement, and the GPU the CPU device, byte for byte on the hosts' synthetic stream, in
    the kernel the header's rule names."""
    n, h, w, c = shape
    host = np.empty(shape, np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, n_threads)
    for k, spec in enumerate(specs):
        want = cpu_run(fam, pkg, L, host, spec, n_threads)
        assert np.array_equal(want, fam.ref(host, spec)), k
        assert np.array_equal(gpu_run(fam, pkg, L, torch, host, spec), want), k
        assert last(L) == fam.kernel(shape, spec), k


def _spoil_map(fam, spec):
    """A spec whose map, if it has one, is a copy that spoil() overwrites: a context must have copied it inside the setter."""
    if fam.fmap(spec) is None:
        return spec, lambda: None
    mine = fam.fmap(spec).copy()

    def spoil():
        mine[:] = 0x7F7F7F7F
    return (mine,) + tuple(spec[1:]), spoil


def check_gpu_context(fam, pkg, L, img, spec, kernel, n_slots=3, repeats=3):
    """A GPU context with the filter set: a pageable submit with 64 guard bytes behind the output; `repeats` pinned submits,
    in place over the host link and one launch each (not the batch server), with at least 4096 guard bytes; the kernel's
    name and bytes_alg = input + output; ERR_UNSUPPORTED from the band, bands and planar submits and both resident runs;
    ERR_STATE on a second set."""
    n, h, w, c = img.shape
    want = fam.ref(img, spec)
    assert kernel == fam.kernel(img.shape, spec)
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=n_slots) as ctx:
        mine, spoil = _spoil_map(fam, spec)
        fam.set(ctx, pkg, mine)
        spoil()
        out = np.full(want.size + 64, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)                  # pageable: the slots hold the larger of the two sizes
        t = ctx.sync()
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()
        assert last(L) == kernel
        assert t["bytes_alg"] == img.size + want.size                   # a map is not counted
        with pinned(L, img.size, want.size + 4096) as ((pin_in, a), (pin_out, b)):
            a[:] = img.reshape(-1)
            z0 = L.mi_blur_zero_copy_launches(ctx.h)
            for _ in range(repeats):
                b[:] = 0xA5
                ctx.submit(pin_in, pin_out, n)
                ctx.sync()
                assert np.array_equal(b[:want.size].reshape(want.shape), want) and (b[want.size:] == 0xA5).all()
            assert L.mi_blur_zero_copy_launches(ctx.h) == z0 + repeats
            assert last(L) == kernel
            assert L.mi_blur_submit_band(ctx.h, pin_in, pin_out, 60, 2, 2) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_submit_bands(ctx.h, pin_in, pin_out, n, h * w * c, 60, 2, 2) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_submit_planar(ctx.h, pin_in, pin_out, n, 0) == pkg.ERR_UNSUPPORTED
            ctx.resident_alloc(2)
            assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
            assert fam.ctx_set(L, ctx.h, fam.host_args(pkg, spec)) == pkg.ERR_STATE


def check_gpu_context_enlarging(fam, pkg, L, img, spec, fill, n_slots=3, repeats=3):
    """An output four times the input, so that slots sized by the input would be overrun: a pageable and `repeats` pinned
    submits with 4096 guard bytes behind the output, one launch each, through the tiled kernel; bytes_alg adds input +
    output per submit, cumulative since the context was made."""
    n, h, w, c = img.shape
    want = fam.ref(img, spec)
    assert want.size == 4 * img.size and fam.takes_tiled(img.shape, spec)
    assert (want != fill).mean() > 0.5                                   # mostly image, not the spec's fill
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=n_slots) as ctx:
        fam.set(ctx, pkg, spec)
        cap = want.size + 4096
        out = np.full(cap, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)                  # pageable
        t = ctx.sync()
        assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()
        assert last(L) == fam.tiled
        assert t["bytes_alg"] == img.size + want.size
        with pinned(L, img.size, cap) as ((pin_in, a), (pin_out, b)):
            a[:] = img.reshape(-1)
            z0 = L.mi_blur_zero_copy_launches(ctx.h)
            for k in range(repeats):
                b[:] = 0xA5
                ctx.submit(pin_in, pin_out, n)
                t = ctx.sync()
                assert np.array_equal(b[:want.size].reshape(want.shape), want) and (b[want.size:] == 0xA5).all()
                assert t["bytes_alg"] == (k + 2) * (img.size + want.size)
            assert L.mi_blur_zero_copy_launches(ctx.h) == z0 + repeats
            assert last(L) == fam.tiled


# ---------------------------------------------------------------- shared bodies: CPU-device contexts
def check_cpu_context(fam, pkg, L, img, spec, n_threads=3):
    """A CPU-device context with the filter set through the bare mi_blur_ctx_set_*, whose structs (and map) are then
    overwritten: the context keeps copies.  One submit into pageable memory with 64 guard bytes either side; bytes_alg =
    input + output (a map is not counted) and the image count; ERR_UNSUPPORTED from the band, bands and planar submits and
    both resident runs, which leave their output untouched; ERR_STATE on a second set."""
    n, h, w, c = img.shape
    want = fam.ref(img, spec)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n, n_threads=n_threads) as ctx:
        mine, spoil = _spoil_map(fam, spec)
        structs = fam.structs(pkg, mine)
        assert fam.ctx_set(L, ctx.h, fam.host_args(pkg, mine, structs)) == pkg.OK
        for s in structs:
            C.memset(C.byref(s), 0xFF, C.sizeof(s))
        spoil()
        out = np.full(want.size + 128, 0xA5, np.uint8)
        ctx.submit(img.ctypes.data, out.ctypes.data + 64, n)
        t = ctx.sync()
        assert np.array_equal(out[64:64 + want.size].reshape(want.shape), want)
        assert (out[:64] == 0xA5).all() and (out[64 + want.size:] == 0xA5).all()
        assert t["bytes_alg"] == img.size + want.size and t["images"] == n
        o = np.zeros_like(img)
        assert L.mi_blur_submit_band(ctx.h, img.ctypes.data, o.ctypes.data, 20, 2, 2) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_submit_bands(ctx.h, img.ctypes.data, o.ctypes.data, n, h * w * c, 20, 2, 2) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_submit_planar(ctx.h, img.ctypes.data, o.ctypes.data, n, 0) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_resident_run(ctx.h, 1, 1, 0) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_resident_run_fused(ctx.h, 1, 1, 0) == pkg.ERR_UNSUPPORTED
        assert not o.any()
        assert fam.ctx_set(L, ctx.h, fam.host_args(pkg, spec)) == pkg.ERR_STATE


def check_setters_replace_each_other(pkg, L, img, sequences):
    """A context holds one filter: each set_* replaces what another set before.  sequences: (setters, want) pairs; the
    setters (callables on the context) run in that order on a fresh CPU-device context, whose submit then gives `want`,
    the last one's output, inside 64 guard bytes, and counts input + output bytes."""
    n, h, w, c = img.shape
    for setters, want in sequences:
        with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
            for s in setters:
                s(ctx)
            out = np.full(want.size + 64, 0xA5, np.uint8)
            ctx.submit(img.ctypes.data, out.ctypes.data, n)
            t = ctx.sync()
            assert np.array_equal(out[:want.size].reshape(want.shape), want) and (out[want.size:] == 0xA5).all()
            assert t["bytes_alg"] == img.size + want.size               # for a filter that keeps the size: twice the input


# ---------------------------------------------------------------- shared bodies: refused arguments
# Every row is (w, h, c, args): args as Resampler.args() gives them.  The calls are made on an 8 x 8 x 3 input and a
# 16 x 16 x 3 output buffer, so `good` has an output of at most 16 x 16.
def size_rows(mk, rest=()):
    """The rows of the four families whose struct holds an output size and a mode.  mk(wo=16, ho=16, mode=...) -> the struct;
    rest: the arguments after it (remap's map)."""
    row = lambda w, h, c, **kw: (w, h, c, (C.byref(mk(**kw)),) + tuple(rest))
    rows = [row(w, h, c) for w, h, c in [(0, 8, 3), (8, 0, 3), (8, 8, 0), (-1, 8, 3), (MAX_DIM + 1, 1, 1), (1, MAX_DIM + 1, 1)]]
    rows += [row(8, 8, 3, **kw) for kw in [dict(wo=0), dict(ho=0), dict(wo=-3), dict(ho=-1), dict(wo=MAX_DIM + 1, ho=1), dict(wo=1, ho=MAX_DIM + 1),
                                            dict(mode=2), dict(mode=-1)]]
    rows.append(row(8, 8, 3, wo=MAX_DIM, ho=MAX_DIM))                   # the output image: 3 GiB, over the per-image limit
    rows.append(row(8, 8, 40000, wo=MAX_DIM, ho=1))                     # the output row: over INT_MAX / 2
    return rows


def sampler_rows(mk, rest=()):
    """The rows of the three samplers (warp, perspective, remap): border and fill."""
    return [(8, 8, 3, (C.byref(mk(**kw)),) + tuple(rest)) for kw in [dict(border=2), dict(border=-1), dict(fill=-1), dict(fill=256)]]


def bad_calls(pkg, call, good, rows):
    """call(in, out, w, h, c, args) -> status, for every argument set the header calls invalid: each argument of `good` null
    in turn, a null input, a null output, the input as the output, and every row of `rows`: a list, or a function of the
    output buffer's address that gives one (remap: a map that is the output).  Returns the two buffers."""
    a = np.zeros((8, 8, 3), np.uint8)
    b = np.zeros((16, 16, 3), np.uint8)
    ia, ib = a.ctypes.data, b.ctypes.data
    rows = rows(ib) if callable(rows) else rows
    bad = [(ia, ib, 8, 8, 3, good[:j] + (None,) + good[j + 1:]) for j in range(len(good))]
    bad += [(None, ib, 8, 8, 3, good), (ia, None, 8, 8, 3, good), (ia, ia, 8, 8, 3, good)]
    bad += [(ia, ib) + tuple(r) for r in rows]
    for k, (i, o, w, h, c, args) in enumerate(bad):
        assert call(i, o, w, h, c, args) == pkg.ERR_INVALID, (k - len(bad) + len(rows), w, h, c)       # the index in `rows`, negative for the rows above
    return a, b


def check_cpu_run_refuses(fam, pkg, L, good, rows):
    """mi_blur_cpu_run_*: bad_calls(), n_images == -1; a good call and an empty batch are MI_BLUR_OK."""
    a, b = bad_calls(pkg, lambda i, o, w, h, c, args: fam.cpu_run(L, i, o, w, h, c, 1, args, 1), good, rows)
    run = lambda n: fam.cpu_run(L, a.ctypes.data, b.ctypes.data, 8, 8, 3, n, good, 1)
    assert run(-1) == pkg.ERR_INVALID
    assert run(1) == pkg.OK and run(0) == pkg.OK
    return a, b


def check_enqueue_invalid_before_no_device(fam, pkg, L, good, rows):
    """mi_blur_enqueue_*: every argument is checked before a device is asked for; without a GPU a good call is
    ERR_NO_DEVICE (with one, the null stream of an empty batch is MI_BLUR_OK)."""
    a, b = bad_calls(pkg, lambda i, o, w, h, c, args: fam.enqueue(L, i, o, w, h, c, 1, args, None), good, rows)
    run = lambda n: fam.enqueue(L, a.ctypes.data, b.ctypes.data, 8, 8, 3, n, good, None)
    assert run(-1) == pkg.ERR_INVALID
    if L.mi_blur_device_count() <= 0:
        assert run(1) == pkg.ERR_NO_DEVICE and run(0) == pkg.ERR_NO_DEVICE
    else:
        assert run(0) == pkg.OK


def check_ctx_set_refuses(fam, pkg, L, good, bad):
    """mi_blur_ctx_set_* on an 8 x 8 x 3 CPU-device context: a null context or argument is ERR_INVALID whatever the state,
    an invalid struct (`bad`: args tuples) ERR_INVALID before the first submit, anything ERR_STATE after it; the refused
    sets leave the box blur in place; a context whose own size is over MAX_DIM takes none of these filters."""
    nulls = [good[:j] + (None,) + good[j + 1:] for j in range(len(good))]
    with pkg.Context(pkg.DEVICE_CPU, 8, 8, 3, 1, max_batch=1) as ctx:
        assert fam.ctx_set(L, None, good) == pkg.ERR_INVALID
        for k, args in enumerate(nulls + list(bad)):
            assert fam.ctx_set(L, ctx.h, args) == pkg.ERR_INVALID, k - len(nulls)
        img = np.random.default_rng(2).integers(0, 256, size=(1, 8, 8, 3), dtype=np.uint8)
        out, box = np.empty_like(img), np.empty_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, 1)
        t = ctx.sync()
        assert L.mi_blur_cpu_run(img.ctypes.data, box.ctypes.data, 8, 8, 3, 1, 1, 1) == pkg.OK
        assert np.array_equal(out, box) and t["bytes_alg"] == 2 * img.size
        assert fam.ctx_set(L, ctx.h, good) == pkg.ERR_STATE
        assert fam.ctx_set(L, ctx.h, bad[0]) == pkg.ERR_STATE
        for args in nulls:
            assert fam.ctx_set(L, ctx.h, args) == pkg.ERR_INVALID
    with pkg.Context(pkg.DEVICE_CPU, MAX_DIM + 1, 2, 1, 1, max_batch=1) as wide:
        assert fam.ctx_set(L, wide.h, good) == pkg.ERR_INVALID
