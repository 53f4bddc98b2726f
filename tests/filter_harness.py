"""What the per-family test files (tests/test_{sep,median,morph,bilateral,conv}_{gpu,host}.py, tests/test_narrow_rows_gpu.py,
tests/test_kernel_proofs_gpu.py, tests/test_large_shapes_gpu.py) share (not a test module, and not a conftest: fixtures reach a test file by plain import into its namespace).

A Family holds what the families differ in: where each export wants the filter spliced into its argument list, the
Context setter, the kernel names, the vertical halo and the numpy restatement.  A filter value is what those exports take:
a SepKernel, a median radius, an (op, rx, ry) triple, a Bilateral, a Conv.  gpu_run / dev_run / cpu_run launch one filter
through the C ABI; the check_* functions are the bodies the family files had in common.  They take the family, one image and one
filter (a list where a large buffer is shared) and every number the families' copies differed in; the loops over shapes,
radii and tables, and the seeds, stay in the family files."""
import ctypes as C
import os
import typing

import numpy as np
import pytest

import conv_ref as cr
import kernel_proofs as kp
from bilateral_ref import ref_bilateral
from median_ref import ref_median
from morph_ref import ref_morph
from sep_ref import ref_sep

TILE_ROWS, TILE_CHUNKS = 32, 32                                   # the bilateral and conv tiled kernels' tile: output rows x 16-byte chunk columns


# ---------------------------------------------------------------- fixtures and files
@pytest.fixture(scope="module")
def torch_cuda(L):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    assert L.mi_blur_device_count() >= 1, "libmi_blur.so sees no HIP device"
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def apps(pkg):
    pkg.build_native()
    return os.path.join(pkg.APPS, "heterogeneous_blur"), os.path.join(pkg.APPS, "split_image_blur")


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


# ---------------------------------------------------------------- the families
class Family(typing.NamedTuple):
    name: str
    enqueue: typing.Callable        # (L, d_in, d_out, w, h, c, n, filt, stream) -> status
    enqueue_band: typing.Callable   # (L, d_in, d_out, w, h, c, y0, y1, filt, stream) -> status
    cpu_run: typing.Callable        # (L, in, out, w, h, c, n, filt, n_threads) -> status
    ctx_set: typing.Callable        # (L, context handle, filt) -> status: the bare mi_blur_ctx_set_* call
    set: typing.Callable            # (Context, filt): Context.set_*, which raises on a status
    fast: str                       # the kernel of rows of whole 16-byte chunks with 1-4 channels at aligned pointers ...
    generic: str                    # ... and of everything else
    halo: typing.Callable           # filt -> rows a band needs above and below
    ref: typing.Callable            # (img N x H x W x C, filt) -> the numpy restatement
    takes_fast: typing.Callable = lambda filt: True

    def kernel(self, filt, aligned=True):
        return self.fast if aligned and self.takes_fast(filt) else self.generic


def _ref(k):
    return None if k is None else C.byref(k)


def _struct_family(name, setter, halo, ref):
    """sep, bilateral and conv take their filter as a struct by reference: after the image count, after the band's rows."""
    return Family(
        name,
        enqueue=lambda L, i, o, w, h, c, n, k, s: getattr(L, f"mi_blur_enqueue_{name}")(i, o, w, h, c, n, _ref(k), s),
        enqueue_band=lambda L, i, o, w, h, c, y0, y1, k, s: getattr(L, f"mi_blur_enqueue_{name}_band")(i, o, w, h, c, y0, y1, _ref(k), s),
        cpu_run=lambda L, i, o, w, h, c, n, k, nt: getattr(L, f"mi_blur_cpu_run_{name}")(i, o, w, h, c, n, _ref(k), nt),
        ctx_set=lambda L, ctx, k: getattr(L, f"mi_blur_ctx_set_{setter}")(ctx, _ref(k)),
        set=lambda ctx, k: getattr(ctx, f"set_{setter}")(k),
        fast=f"blur_{name}_tiled_kernel", generic=f"blur_{name}_generic_kernel", halo=halo, ref=ref)


def _bilateral_tables(k):
    n = 2 * k.radius + 1
    return np.array(k.spatial[:n * n]).reshape(n, n), np.array(k.range[:])


SEP = _struct_family("sep", "kernel", lambda k: k.ry, lambda img, k: ref_sep(img, *k.taps()))
BILATERAL = _struct_family("bilateral", "bilateral", lambda k: k.radius, lambda img, k: ref_bilateral(img, *_bilateral_tables(k)))
CONV = _struct_family("conv", "conv", lambda k: k.ry, lambda img, k: cr.ref_conv(img, k.taps()[0], k.shift, k.bias, cr.MODES[k.mode], k.taps()[1]))
MEDIAN = Family(
    "median",
    enqueue=lambda L, i, o, w, h, c, n, r, s: L.mi_blur_enqueue_median(i, o, w, h, c, r, n, s),
    enqueue_band=lambda L, i, o, w, h, c, y0, y1, r, s: L.mi_blur_enqueue_median_band(i, o, w, h, c, r, y0, y1, s),
    cpu_run=lambda L, i, o, w, h, c, n, r, nt: L.mi_blur_cpu_run_median(i, o, w, h, c, r, n, nt),
    ctx_set=lambda L, ctx, r: L.mi_blur_ctx_set_median(ctx, r),
    set=lambda ctx, r: ctx.set_median(r),
    fast="blur_median_fast_kernel", generic="blur_median_generic_kernel", halo=lambda r: r, ref=ref_median,
    takes_fast=lambda r: r <= 2)
MORPH = Family(
    "morph",
    enqueue=lambda L, i, o, w, h, c, n, f, s: L.mi_blur_enqueue_morph(i, o, w, h, c, *f, n, s),
    enqueue_band=lambda L, i, o, w, h, c, y0, y1, f, s: L.mi_blur_enqueue_morph_band(i, o, w, h, c, *f, y0, y1, s),
    cpu_run=lambda L, i, o, w, h, c, n, f, nt: L.mi_blur_cpu_run_morph(i, o, w, h, c, *f, n, nt),
    ctx_set=lambda L, ctx, f: L.mi_blur_ctx_set_morph(ctx, *f),
    set=lambda ctx, f: ctx.set_morph(*f),
    fast="blur_morph_tiled_kernel", generic="blur_morph_generic_kernel", halo=lambda f: f[2], ref=lambda img, f: ref_morph(img, *f))


# ---------------------------------------------------------------- one launch
def gpu_run(family, pkg, L, torch, host, filt, offset_in=0, offset_out=0, y0=None, y1=None):
    """host: N x H x W x C -> mi_blur_enqueue_* (or *_band for one image with y0/y1).  The input lies offset_in bytes into
    a buffer with 64 spare bytes, the output offset_out bytes into one with 128 bytes of 0x5A to spare: guards either side."""
    n, h, w, c = host.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size_out = n * (y1 - y0) * w * c
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = family.enqueue(L, d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, filt, s)
    else:
        assert n == 1
        rc = family.enqueue_band(L, d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, y0, y1, filt, s)
    pkg.check(rc, f"mi_blur_enqueue_{family.name}")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, y1 - y0, w, c)


DEV_GUARD = 256


def dev_run(family, pkg, L, torch, d_img, filt, y0=None, y1=None):
    """d_img (N, H, W, C) uint8 on the device -> mi_blur_enqueue_* (or *_band for one image with y0 / y1), the output left
    on the device: for sweeps of many small launches over one upload.  DEV_GUARD bytes of 0x5A either side of the output."""
    n, h, w, c = d_img.shape
    y0 = 0 if y0 is None else y0
    y1 = h if y1 is None else y1
    size = n * (y1 - y0) * w * c
    out = torch.full((size + 2 * DEV_GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if y0 == 0 and y1 == h:
        rc = family.enqueue(L, d_img.data_ptr(), out.data_ptr() + DEV_GUARD, w, h, c, n, filt, s)
    else:
        assert n == 1
        rc = family.enqueue_band(L, d_img.data_ptr(), out.data_ptr() + DEV_GUARD, w, h, c, y0, y1, filt, s)
    pkg.check(rc, f"mi_blur_enqueue_{family.name}")
    torch.cuda.synchronize()
    assert bool((out[:DEV_GUARD] == 0x5A).all()) and bool((out[DEV_GUARD + size:] == 0x5A).all()), "wrote outside the output"
    return out[DEV_GUARD:DEV_GUARD + size].reshape(n, y1 - y0, w, c)


def cpu_run(family, pkg, L, img, filt, n_threads, prefill=True):
    """img: N x H x W x C -> mi_blur_cpu_run_*.  The host files' output starts as 0xA5, so a byte left unwritten shows."""
    a = np.ascontiguousarray(img)
    out = np.full_like(a, 0xA5) if prefill else np.empty_like(a)
    n, h, w, c = a.shape
    pkg.check(family.cpu_run(L, a.ctypes.data, out.ctypes.data, w, h, c, n, filt, n_threads), f"mi_blur_cpu_run_{family.name}")
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


# ---------------------------------------------------------------- shared bodies: GPU
def check_gpu_context(family, pkg, L, img, filt, pinned_repeats, n_slots=3, bands=(60, 180), band=(1, 50, 150)):
    """Every submit form of a GPU context takes the filter: pageable, pinned (in place over the host link, one launch per
    submit: not the batch server), strided bands (rows `bands` of every image with halo rows, into the same rows of the
    output), one band (image, rows), planar.  Then ERR_STATE on a second set and ERR_UNSUPPORTED from both resident runs."""
    n, h, w, c = img.shape
    r, want, kernel = family.halo(filt), family.ref(img, filt), family.kernel(filt)
    pitch, isz = w * c, img[0].size
    with pkg.Context(0, w, h, c, 1, max_batch=n, n_slots=n_slots) as ctx:
        family.set(ctx, filt)
        out = np.zeros_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(out, want)
        assert L.mi_blur_last_kernel().decode() == kernel
        pin_in, pin_out = L.mi_blur_host_alloc(img.size), L.mi_blur_host_alloc(img.size)
        try:
            a = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_in)).reshape(img.shape)
            b = np.ctypeslib.as_array((C.c_uint8 * img.size).from_address(pin_out)).reshape(img.shape)
            a[:] = img
            z0 = L.mi_blur_zero_copy_launches(ctx.h)
            for _ in range(pinned_repeats):
                b[:] = 0
                ctx.submit(pin_in, pin_out, n)
                ctx.sync()
                assert np.array_equal(b, want)
            assert L.mi_blur_zero_copy_launches(ctx.h) == z0 + pinned_repeats
            assert L.mi_blur_last_kernel().decode() == kernel
        finally:
            L.mi_blur_host_free(pin_in)
            L.mi_blur_host_free(pin_out)
        y0, y1 = bands
        bo = np.zeros_like(img)
        ctx.submit_bands(img.ctypes.data + (y0 - r) * pitch, bo.ctypes.data + y0 * pitch, n, isz, y1 - y0 + 2 * r, r, r)
        ctx.sync()
        assert np.array_equal(bo[:, y0:y1], want[:, y0:y1]) and not bo[:, :y0].any() and not bo[:, y1:].any()
        i, y0, y1 = band
        so = np.zeros((y1 - y0, w, c), np.uint8)
        ctx.submit_band(img[i].ctypes.data + (y0 - r) * pitch, so.ctypes.data, y1 - y0 + 2 * r, r, r)
        ctx.sync()
        assert np.array_equal(so, want[i, y0:y1])
        planar = np.ascontiguousarray(img.transpose(0, 3, 1, 2))
        po = np.zeros_like(img)
        ctx.submit_planar(planar.ctypes.data, po.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(po, want)
        assert family.ctx_set(L, ctx.h, filt) == pkg.ERR_STATE
        ctx.resident_alloc(2)
        assert L.mi_blur_resident_run(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_resident_run_fused(ctx.h, 2, 1, 0) == pkg.ERR_UNSUPPORTED


def check_gpu_band_split_equals_whole(family, pkg, L, torch, img, filt, whole, splits):
    """One image cut at each row of `splits`, each part launched as a band with the filter's halo (no rows above row 0:
    the bottom part of a split less than a halo below the top starts at row 0), joined: the whole image."""
    h, ry = img.shape[1], family.halo(filt)
    for split in splits:
        top_rows = min(h, split + ry)
        top = gpu_run(family, pkg, L, torch, np.ascontiguousarray(img[:, :top_rows]), filt, y0=0, y1=split)
        b0 = max(split - ry, 0)
        bot = gpu_run(family, pkg, L, torch, np.ascontiguousarray(img[:, b0:]), filt, y0=split - b0, y1=h - b0)
        assert np.array_equal(np.concatenate([top, bot], axis=1), whole), (family.name, img.shape, filt, split)


def check_bands_inside_the_image(family, pkg, L, torch, img, filt, skip_empty=False):
    """Bands of one image against the same rows of the whole image's restatement: away from both edges by the halo, the top
    half, the bottom two thirds, one row; then a band split at the halo (at least 1), the middle and as far from the end."""
    h, ry = img.shape[1], family.halo(filt)
    whole = family.ref(img, filt)
    for y0, y1 in ((ry, h - ry), (0, h // 2), (h // 3, h), (5, 6)):
        if skip_empty and y0 >= y1:
            continue
        got = gpu_run(family, pkg, L, torch, img, filt, y0=y0, y1=y1)
        assert np.array_equal(got, whole[:, y0:y1]), (family.name, img.shape, filt, y0, y1)
    check_gpu_band_split_equals_whole(family, pkg, L, torch, img, filt, whole, (max(ry, 1), h // 2, h - max(ry, 1)))


def check_unaligned_pointers(family, pkg, L, torch, img, filt, aligned_first=True, offsets=((1, 0), (0, 7), (3, 5))):
    """An input or output pointer off 16 bytes takes the generic kernel and gives the same bytes, guards intact."""
    want = family.ref(img, filt)
    if aligned_first:
        assert np.array_equal(gpu_run(family, pkg, L, torch, img, filt), want)
        assert L.mi_blur_last_kernel().decode() == family.kernel(filt)
    for oi, oo in offsets:
        assert np.array_equal(gpu_run(family, pkg, L, torch, img, filt, oi, oo), want), (family.name, filt, oi, oo)
        assert L.mi_blur_last_kernel().decode() == family.generic


def check_batch_over_2gib(family, pkg, L, torch, img, filters, n, same, patch_last=True, check_kernel=True):
    """A batch of more than 2^31 bytes (n copies of img): 64-bit image offsets, 32-bit offsets inside an image.  The
    images `same` against img's restatement; with patch_last the last image differs from the others and is checked too."""
    h, w, c = img.shape[1:]
    d_in = torch.from_numpy(img[0]).cuda().unsqueeze(0).repeat(n, 1, 1, 1)
    if patch_last:
        d_in[n - 1, 100:200, 300:400] = 255
        last = d_in[n - 1].cpu().numpy()[None]
    d_out = torch.zeros_like(d_in)
    for filt in filters:
        pkg.check(family.enqueue(L, d_in.data_ptr(), d_out.data_ptr(), w, h, c, n, filt, None))
        torch.cuda.synchronize()
        if check_kernel:
            assert L.mi_blur_last_kernel().decode() == family.kernel(filt)
        want0 = torch.from_numpy(family.ref(img, filt)[0]).cuda()
        for i in same:
            assert bool((d_out[i] == want0).all()), (family.name, filt, i)
        if patch_last:
            assert np.array_equal(d_out[n - 1].cpu().numpy(), family.ref(last, filt)[0]), (family.name, filt)
    del d_in, d_out
    torch.cuda.empty_cache()


def check_synthetic_stream(family, pkg, L, torch, filters, shape, fill_threads, cpu_threads, check_kernel=False):
    """The GPU and the CPU device agree byte for byte on the hosts' synthetic stream."""
    n, h, w, c = shape
    host = np.empty(shape, np.uint8)
    L.mi_blur_fill_synthetic(host.ctypes.data, w, h, c, 0, n, fill_threads)
    for filt in filters:
        want = cpu_run(family, pkg, L, host, filt, cpu_threads, prefill=False)
        assert np.array_equal(gpu_run(family, pkg, L, torch, host, filt), want), (family.name, filt)
        if check_kernel:
            assert L.mi_blur_last_kernel().decode() == family.kernel(filt)


# ---------------------------------------------------------------- shared bodies: tile geometry of the tiled kernels
# The sep, morph, bilateral and conv tiled kernels cut a launch into the same tiles (fill_tiles, kernel_common.h): TILE_ROWS
# output rows x at most TILE_CHUNKS chunk columns, one workgroup each; from 16 workgroups on, the block -> tile remap is on.
GEOMETRY_CPR = (1, 2, 3, 31, 32, 33, 64, 65, 97)                 # chunks per row, rounded to what whole pixels fill (kp.chunk_cols)
GEOMETRY_ROWS = (1, 2, 7, 8, 9, 31, 32, 33, 64, 65)
BAND_H, BAND_CPR = 130, (2, 33)
BAND_Y0 = (0, 1, 31, 32, 33, 63, 64, 65)
GRID_BATCHES = ((2, 32, 32), (15, 32, 32), (16, 32, 32), (3, 65, 65), (5, 33, 1), (9, 31, 33))     # (images, rows, chunks per row)
REMAP_BLOCKS = 16


def band_y1(y0, h=BAND_H):
    return sorted({y0 + 1, 64, 65, 96, 97, h} - set(range(y0 + 1)))


def tile_blocks(n, rows, cpr):
    return n * -(-rows // TILE_ROWS) * -(-cpr // TILE_CHUNKS)


def random_bytes(rng, n, h, w, c):
    return rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)


def check_tiled_geometry_sweep(family, pkg, L, torch, rng, c, make_image, make_filter, n_edges):
    """Every chunk count of GEOMETRY_CPR x every row count of GEOMETRY_ROWS for c channels, one image each, through the
    tiled kernel.  make_filter(q) -> (filter, the kernel's bucket edges it sits on) for the q-th shape: the filter walks
    its kernel's own edges as the shapes go by, and all n_edges combinations must have occurred."""
    seen = set()
    for i, cpr in enumerate(GEOMETRY_CPR):
        w = kp.chunk_cols(cpr, c) * 16 // c
        for j, rows in enumerate(GEOMETRY_ROWS):
            filt, edge = make_filter(i * len(GEOMETRY_ROWS) + j)
            seen.add(edge)
            img = make_image(rng, 1, rows, w, c)
            got = dev_run(family, pkg, L, torch, torch.from_numpy(img).cuda(), filt).cpu().numpy()
            assert L.mi_blur_last_kernel().decode() == family.fast, (family.name, c, cpr, rows, edge)
            assert np.array_equal(got, family.ref(img, filt)), (family.name, c, cpr, rows, edge)
    assert len(seen) == n_edges, (family.name, c, sorted(seen))


def check_bands_and_grids(family, pkg, L, torch, rng, make_image, band_filters, grid_filter, channels=(1, 2, 3, 4)):
    """Bands of one image of BAND_H rows whose y0 / y1 sit on and next to tile boundaries (multiples of TILE_ROWS), on rows
    of 2 and of 33 chunks, against the same rows of the whole image's restatement; then batches whose grid is below and
    at or above REMAP_BLOCKS workgroups (the XCD remap off and on), both sides for every channel count.  band_filters:
    callables rng -> filter, each called once per image, after the image is drawn; grid_filter likewise, per batch."""
    for c in channels:
        for cpr in BAND_CPR:
            w = kp.chunk_cols(cpr, c) * 16 // c
            img = make_image(rng, 1, BAND_H, w, c)
            d_img = torch.from_numpy(img).cuda()
            for make in band_filters:
                filt = make(rng)
                whole = family.ref(img, filt)
                for y0 in BAND_Y0:
                    for y1 in band_y1(y0):
                        got = dev_run(family, pkg, L, torch, d_img, filt, y0, y1).cpu().numpy()
                        assert L.mi_blur_last_kernel().decode() == family.fast
                        assert np.array_equal(got, whole[:, y0:y1]), (family.name, c, cpr, y0, y1)
    sides = set()
    for c in channels:
        for n, rows, cpr in GRID_BATCHES:
            w = kp.chunk_cols(cpr, c) * 16 // c
            nb = tile_blocks(n, rows, kp.chunk_cols(cpr, c))
            sides.add((c, nb >= REMAP_BLOCKS))
            img = make_image(rng, n, rows, w, c)
            filt = grid_filter(rng)
            got = dev_run(family, pkg, L, torch, torch.from_numpy(img).cuda(), filt).cpu().numpy()
            assert L.mi_blur_last_kernel().decode() == family.fast
            assert np.array_equal(got, family.ref(img, filt)), (family.name, c, n, rows, cpr, nb)
    assert len(sides) == 2 * len(channels)


# ---------------------------------------------------------------- shared bodies: CPU-device contexts
def check_cpu_context(family, pkg, L, img, filt, ctx_kw, halos=None, rows=(10, 30), spoil=None):
    """Every submit form of a CPU-device context takes the filter: whole images, one band (`rows` of image 0 with halo rows:
    clamping at the band's own edges, interior rows only), the same band of every image, strided, and planar in.  Then
    ERR_STATE on a second set and ERR_UNSUPPORTED from both resident runs.  halos: (top, bottom), the filter's own halo if
    None.  spoil(k): the context is set from a duplicate of the struct, which spoil then damages: the context keeps a copy."""
    n, h, w, c = img.shape
    top, bot = halos or (family.halo(filt),) * 2
    want = family.ref(img, filt)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n, **ctx_kw) as ctx:
        if spoil is None:
            family.set(ctx, filt)
        else:
            k = type(filt).from_buffer_copy(filt)
            family.set(ctx, k)
            spoil(k)
        out = np.zeros_like(img)
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(out, want)
        y0, y1 = rows
        nrows = y1 - y0
        band = np.ascontiguousarray(img[0, y0:y1])
        bo = np.zeros((nrows - top - bot, w, c), np.uint8)
        ctx.submit_band(band.ctypes.data, bo.ctypes.data, nrows, top, bot)
        ctx.sync()
        assert np.array_equal(bo, family.ref(band[None], filt)[0, top:nrows - bot])
        bs = np.zeros_like(img)
        pitch = w * c
        ctx.submit_bands(img.ctypes.data + y0 * pitch, bs.ctypes.data + (y0 + top) * pitch, n, h * pitch, nrows, top, bot)
        ctx.sync()
        assert np.array_equal(bs[:, y0 + top:y1 - bot], family.ref(img[:, y0:y1], filt)[:, top:nrows - bot])
        planar = np.ascontiguousarray(img.transpose(0, 3, 1, 2))
        po = np.zeros_like(img)
        ctx.submit_planar(planar.ctypes.data, po.ctypes.data, n)
        ctx.sync()
        assert np.array_equal(po, want)
        assert family.ctx_set(L, ctx.h, filt) == pkg.ERR_STATE             # after the first submit
        assert L.mi_blur_resident_run(ctx.h, 1, 1, 0) == pkg.ERR_UNSUPPORTED
        assert L.mi_blur_resident_run_fused(ctx.h, 1, 1, 0) == pkg.ERR_UNSUPPORTED


def check_cpu_band_split_equals_whole(family, pkg, L, img, filt, splits, ctx_kw):
    """One image (1 x H x W x C) cut at each row of `splits`, both parts submitted as bands with the filter's halo, joined:
    the whole image's restatement."""
    h, w, c = img.shape[1:]
    ry = family.halo(filt)
    whole = family.ref(img, filt)
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=1, **ctx_kw) as ctx:
        family.set(ctx, filt)
        for split in splits:
            top_rows = min(h, split + ry)
            top_in = np.ascontiguousarray(img[0, :top_rows])
            top = np.zeros((split, w, c), np.uint8)
            ctx.submit_band(top_in.ctypes.data, top.ctypes.data, top_rows, 0, top_rows - split)
            b0 = max(split - ry, 0)
            bot_in = np.ascontiguousarray(img[0, b0:])
            bot = np.zeros((h - split, w, c), np.uint8)
            ctx.submit_band(bot_in.ctypes.data, bot.ctypes.data, h - b0, split - b0, 0)
            ctx.sync()
            assert np.array_equal(np.concatenate([top, bot]), whole[0]), (family.name, filt, split)


def check_set_rules_order(family, pkg, L, img, sequences, refused, good):
    """A context holds one filter: each set_* replaces what another set before.  sequences: tuples of (Family, filter), set in
    that order on a fresh CPU-device context; the submit then gives the last one's output: the numpy restatement where it
    is `family`, mi_blur_cpu_run_* on one thread where it is another.  Then, on one more context: every filter of `refused`
    and a null handle are ERR_INVALID and leave the box blur in place, and `good` after the first submit is ERR_STATE."""
    n, h, w, c = img.shape
    by_the_library = {}
    for seq in sequences:
        with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
            for fam, filt in seq:
                fam.set(ctx, filt)
            out = np.zeros_like(img)
            ctx.submit(img.ctypes.data, out.ctypes.data, n)
            ctx.sync()
        fam, filt = seq[-1]
        if fam is family:
            want = family.ref(img, filt)
        else:
            if (fam.name, id(filt)) not in by_the_library:
                by_the_library[fam.name, id(filt)] = cpu_run(fam, pkg, L, img, filt, 1, prefill=False)
            want = by_the_library[fam.name, id(filt)]
        assert np.array_equal(out, want), [f.name for f, _ in seq]
    with pkg.Context(pkg.DEVICE_CPU, w, h, c, 1, max_batch=n) as ctx:
        for bad in refused:
            assert family.ctx_set(L, ctx.h, bad) == pkg.ERR_INVALID, bad
        assert family.ctx_set(L, None, good) == pkg.ERR_INVALID
        out = np.zeros_like(img)                                 # refused calls left the box blur in place
        ctx.submit(img.ctypes.data, out.ctypes.data, n)
        ctx.sync()
        box = np.empty_like(img)
        assert L.mi_blur_cpu_run(img.ctypes.data, box.ctypes.data, w, h, c, 1, n, 1) == pkg.OK
        assert np.array_equal(out, box)
        assert family.ctx_set(L, ctx.h, good) == pkg.ERR_STATE
