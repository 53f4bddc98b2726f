"""The histogram family on the GPU (mi_blur_enqueue_hist, mi_blur_enqueue_tables, mi_blur_enqueue_tone, histogram() and
its kin): exact counts, exact tables and exact bytes against hist_ref.py and the CPU device, and which kernel took each
launch."""
import ctypes as C

import numpy as np
import pytest

from color_ref import ref_preset
from hist_ref import (BINS, EQUALIZE, HIST_GENERIC, HIST_TILED, IMAGE_BLOCKS, RUN, STRETCH, TABLES_GENERIC, TABLES_TILED, blocks, hist_blocks, ref_apply,
                      ref_hist, ref_tone, takes_tiled)
from resample_harness import last, torch_cuda  # noqa: F401
from table_harness import Guarded, stream, upload

pytestmark = pytest.mark.gpu

ONES = 0xFFFFFFFF
# (H, W) whose pixel counts bracket the kernels' units: one group; one group below, at and one above a workgroup's run;
# two workgroups plus one group; 2 x 24, whose rows are not whole chunks for C = 1 and 3 (tiled all the same: the rule is flat)
UNITS = [(4, 4), (RUN - 1, 16), (RUN, 16), (RUN + 1, 16), (2 * RUN + 1, 16), (2, 24)]
UNIT_BLOCKS = (1, 1, 1, 2, 3, 1)


def hist_on_device(pkg, L, torch, ptr, shape):
    """mi_blur_enqueue_hist on the images at ptr into a buffer of 0xFFFFFFFF words with 32 more behind it: the histogram is
    overwritten, not added to, and the words behind it stay."""
    n, h, w, c = shape
    words = n * c * BINS
    d_hist = Guarded(torch, words, "the histogram", np.uint32, ONES, back=32)
    pkg.check(L.mi_blur_enqueue_hist(ptr, d_hist.ptr, w, h, c, n, stream(torch)), "mi_blur_enqueue_hist")
    torch.cuda.synchronize()
    return d_hist.payload().reshape(n, c, BINS)


def gpu_hist(pkg, L, torch, host, offset_in=0):
    d, ptr = upload(torch, host, offset_in)
    return hist_on_device(pkg, L, torch, ptr, host.shape)


def gpu_tables(pkg, L, torch, host, tables, offset_in=0, offset_out=0, offset_tab=0):
    """mi_blur_enqueue_tables: the output lies offset_out bytes into a buffer of 0x5A with 128 bytes to spare."""
    n, h, w, c = host.shape
    d_in, p_in = upload(torch, host, offset_in)
    d_tab, p_tab = upload(torch, np.ascontiguousarray(tables, dtype=np.uint8), offset_tab)
    d_out = Guarded(torch, host.size, "the output", front=offset_out, back=128 - offset_out)
    pkg.check(L.mi_blur_enqueue_tables(p_in, d_out.ptr, w, h, c, n, p_tab, stream(torch)), "mi_blur_enqueue_tables")
    torch.cuda.synchronize()
    return d_out.payload().reshape(host.shape)


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_hist_at_the_kernels_units(pkg, L, torch_cuda, c):
    rng = np.random.default_rng(80 + c)
    for i, (h, w) in enumerate(UNITS):
        img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
        assert takes_tiled(img.shape) and blocks(2, h, w) == hist_blocks(2, h, w) == 2 * UNIT_BLOCKS[i]
        got = gpu_hist(pkg, L, torch_cuda, img)
        assert last(L) == HIST_TILED
        assert np.array_equal(got, ref_hist(img)), (c, h, w)


def test_hist_batches_either_side_of_the_xcd_remap(pkg, L, torch_cuda):
    """Grids of 15 and of 18 workgroups: below 16 the blocks take the runs in order, from 16 on through the XCD remap."""
    h, w, c = 3 * RUN, 16, 3
    rng = np.random.default_rng(85)
    for n in (5, 6):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        img[:, :, :, 0] = (img[:, :, :, 0] // 16 + 16 * np.arange(n)[:, None, None]).astype(np.uint8)     # an image's own range: a wrong image shows
        assert hist_blocks(n, h, w) == 3 * n and (hist_blocks(n, h, w) >= 16) == (n == 6)
        got = gpu_hist(pkg, L, torch_cuda, img)
        assert last(L) == HIST_TILED and np.array_equal(got, ref_hist(img)), n


def test_hist_images_of_more_runs_than_workgroups(pkg, L, torch_cuda):
    """An image has at most IMAGE_BLOCKS workgroups: at 256 runs each takes one, at 257 (the last one short) the first takes
    two, at 513 every workgroup takes two and the first three."""
    rng = np.random.default_rng(87)
    for c, n, h, w, groups in ((1, 2, 1024, 2048, IMAGE_BLOCKS * RUN), (3, 2, 18797, 112, (IMAGE_BLOCKS + 1) * RUN - 5),
                               (1, 1, 2052, 2048, (2 * IMAGE_BLOCKS + 1) * RUN)):
        assert h * w == 16 * groups
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        assert hist_blocks(n, h, w) == n * IMAGE_BLOCKS and blocks(n, h, w) == n * -(-groups // RUN)
        got = gpu_hist(pkg, L, torch_cuda, img)
        assert last(L) == HIST_TILED and np.array_equal(got, ref_hist(img)), (c, n, groups)


@pytest.mark.parametrize("c", [2, 3, 4])
def test_hist_channel_picks(pkg, L, torch_cuda, c):
    """Channel ch is the constant 10 + ch: exactly one non-zero bin per channel, equal to W * H."""
    h, w = 40, 48
    img = np.empty((2, h, w, c), np.uint8)
    img[...] = 10 + np.arange(c)
    got = gpu_hist(pkg, L, torch_cuda, img)
    assert last(L) == HIST_TILED
    for ch in range(c):
        want = np.zeros(BINS, np.uint32)
        want[10 + ch] = w * h
        assert np.array_equal(got[0, ch], want) and np.array_equal(got[1, ch], want), ch


def test_hist_flat_and_wide_counts(pkg, L, torch_cuda):
    torch = torch_cuda
    h, w = 4096, 4097
    n_px = h * w
    assert n_px == 16_781_312 and n_px > 1 << 24
    d = torch.full((n_px,), 200, dtype=torch.uint8, device="cuda")
    got = hist_on_device(pkg, L, torch, d.data_ptr(), (1, h, w, 1))
    assert last(L) == HIST_TILED
    want = np.zeros((1, 1, BINS), np.uint32)
    want[0, 0, 200] = n_px
    assert np.array_equal(got, want)
    d[0::2] = 3                                                      # the value alternates between two levels
    d[1::2] = 250
    got = hist_on_device(pkg, L, torch, d.data_ptr(), (1, h, w, 1))
    want[:] = 0
    want[0, 0, 3] = want[0, 0, 250] = n_px // 2
    assert np.array_equal(got, want)
    del d
    # one value per wave-sized stretch (64 lanes x 16 pixels) and channel: whole waves agree, and their neighbours differ
    stretch = 64 * 16
    k = np.arange(512 * 512 // stretch)
    img = np.empty((512 * 512 // stretch, stretch, 3), np.uint8)
    for ch in range(3):
        img[:, :, ch] = ((k * (7 + 2 * ch) + 31 * ch) % 256)[:, None]
    img = img.reshape(1, 512, 512, 3)
    got = gpu_hist(pkg, L, torch, img)
    assert last(L) == HIST_TILED and np.array_equal(got, ref_hist(img))
    assert (got[0] > 0).sum() > 300 and got[0].max() <= 4 * stretch


def test_hist_other_launches_take_the_generic_kernel(pkg, L, torch_cuda):
    rng = np.random.default_rng(86)
    for h, w in ((7, 5), (1, 1), (3, 17)):
        for c in (1, 2, 3, 4):
            img = rng.integers(0, 256, size=(2, h, w, c), dtype=np.uint8)
            assert not takes_tiled(img.shape)
            got = gpu_hist(pkg, L, torch_cuda, img)
            assert last(L) == HIST_GENERIC and np.array_equal(got, ref_hist(img)), (h, w, c)
    img = rng.integers(0, 256, size=(2, 135, 96, 3), dtype=np.uint8)      # 3 workgroups per image in the generic kernel
    want = ref_hist(img)
    assert np.array_equal(gpu_hist(pkg, L, torch_cuda, img), want) and last(L) == HIST_TILED
    for off in (1, 7, 8):
        assert not takes_tiled(img.shape, off)
        assert np.array_equal(gpu_hist(pkg, L, torch_cuda, img, off), want), off
        assert last(L) == HIST_GENERIC, off


def test_hist_image_offsets_are_64_bit(pkg, L, torch_cuda):
    """3 images of 16384 x 16384 x 4: 3 GiB, so the third image starts beyond 2^31.  Filled on the device with a tiled
    4096-byte pattern plus the image index; the expected counts are those of one pattern tile times the tile count."""
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
    got = hist_on_device(pkg, L, torch, d_in.data_ptr(), (n, h, w, c))
    assert last(L) == HIST_TILED
    want = np.empty((n, c, BINS), np.uint32)
    for i in range(n):
        for ch in range(c):
            want[i, ch] = np.bincount((pattern[ch::c] + np.uint8(i)).astype(np.uint8), minlength=BINS) * (isz // 4096)
    assert want.astype(np.uint64).sum() == n * isz and not np.array_equal(want[0], want[2])
    assert np.array_equal(got, want)
    del d_in
    torch.cuda.empty_cache()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_tables_apply(pkg, L, torch_cuda, c):
    """A random permutation per image and channel, on both kernels, and the tiled kernel at its units."""
    rng = np.random.default_rng(90 + c)
    n = 3
    tables = np.stack([np.stack([rng.permutation(BINS) for _ in range(c)]) for _ in range(n)]).astype(np.uint8)
    assert not np.array_equal(tables[0], tables[1])
    img = rng.integers(0, 256, size=(n, 33, 48, c), dtype=np.uint8)
    want = ref_apply(img, tables)
    assert np.array_equal(gpu_tables(pkg, L, torch_cuda, img, tables), want) and last(L) == TABLES_TILED
    assert np.array_equal(gpu_tables(pkg, L, torch_cuda, img, tables, offset_tab=3), want) and last(L) == TABLES_TILED    # tables at any alignment
    for off in ((1, 0), (0, 7), (8, 8)):
        assert not takes_tiled(img.shape, *off)
        assert np.array_equal(gpu_tables(pkg, L, torch_cuda, img, tables, *off), want), off
        assert last(L) == TABLES_GENERIC, off
    odd = rng.integers(0, 256, size=(n, 7, 5, c), dtype=np.uint8)
    assert np.array_equal(gpu_tables(pkg, L, torch_cuda, odd, tables), ref_apply(odd, tables)) and last(L) == TABLES_GENERIC
    for i, (h, w) in enumerate(UNITS):
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        assert blocks(n, h, w) == n * UNIT_BLOCKS[i]
        assert np.array_equal(gpu_tables(pkg, L, torch_cuda, img, tables), ref_apply(img, tables)), (h, w)
        assert last(L) == TABLES_TILED


def test_tables_batches_either_side_of_the_xcd_remap(pkg, L, torch_cuda):
    h, w, c = 3 * RUN, 16, 3
    rng = np.random.default_rng(95)
    for n in (5, 6):
        tables = np.stack([np.stack([rng.permutation(BINS) for _ in range(c)]) for _ in range(n)]).astype(np.uint8)
        img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
        assert np.array_equal(gpu_tables(pkg, L, torch_cuda, img, tables), ref_apply(img, tables)) and last(L) == TABLES_TILED, n


@pytest.mark.parametrize("c", [1, 3, 4])
def test_tone_end_to_end(pkg, L, torch_cuda, c):
    """mi_blur_enqueue_tone = mi_blur_cpu_run_tone = the numpy composition on the synthetic stream plus a low-contrast
    image: every image gets its own tables."""
    torch = torch_cuda
    n, h, w = 5, 240, 320
    img = np.empty((n, h, w, c), np.uint8)
    L.mi_blur_fill_synthetic(img.ctypes.data, w, h, c, 0, 4, 4)
    img[4] = (90 + np.random.default_rng(96).integers(0, 51, size=(h, w, c))).astype(np.uint8)
    words = n * c * BINS
    assert L.mi_blur_tone_work_bytes(c, n) == 5 * words
    d_in, p_in = upload(torch, img)
    for mode, lo, hi in ((EQUALIZE, 0, 0), (STRETCH, 655, 1310)):
        for joint in (0, 1):
            for mask in (0, 1) + ((7,) if c >= 3 else ()):
                tone = pkg.Tone(mode, lo, hi, joint, mask)
                want, want_hist, want_tables = ref_tone(img, mode, lo, hi, joint, mask)
                cpu_out, cpu_work = np.empty_like(img), np.empty(5 * words, np.uint8)
                pkg.check(L.mi_blur_cpu_run_tone(img.ctypes.data, cpu_out.ctypes.data, w, h, c, n, C.byref(tone), cpu_work.ctypes.data, 4), "mi_blur_cpu_run_tone")
                assert np.array_equal(cpu_out, want)
                d_out = torch.full((img.size + 128,), 0x5A, dtype=torch.uint8, device="cuda")
                d_work = torch.full((5 * words + 64,), 0x5A, dtype=torch.uint8, device="cuda")
                pkg.check(L.mi_blur_enqueue_tone(p_in, d_out.data_ptr(), w, h, c, n, C.byref(tone), d_work.data_ptr(), stream(torch)), "mi_blur_enqueue_tone")
                torch.cuda.synchronize()
                assert last(L) == TABLES_TILED
                o, wk = d_out.cpu().numpy(), d_work.cpu().numpy()
                assert (o[img.size:] == 0x5A).all() and (wk[5 * words:] == 0x5A).all()
                assert np.array_equal(wk[:5 * words], cpu_work)
                hist, tables = wk[:4 * words].view(np.uint32).reshape(n, c, BINS), wk[4 * words:5 * words].reshape(n, c, BINS)
                assert np.array_equal(hist, want_hist) and np.array_equal(tables, want_tables)
                got = o[:img.size].reshape(img.shape)
                assert np.array_equal(got, want), (mode, joint, mask)
                # images of one batch get different tables, and each image matches its own
                # (two frames of the synthetic stream differ in their equalisation; their 1 % and 2 % levels are the same)
                assert not np.array_equal(tables[3], tables[4]) and (mode == STRETCH or not np.array_equal(tables[0, 0], tables[1, 0]))
                for i in range(n):
                    assert np.array_equal(got[i], ref_apply(img[i:i + 1], tables[i:i + 1])[0]), i


def test_numpy_functions_on_the_gpu(pkg, L, torch_cuda):
    rng = np.random.default_rng(97)
    stack = rng.integers(0, 256, size=(5, 90, 128, 3), dtype=np.uint8)
    stack[3] = (40 + stack[3] % 120).astype(np.uint8)
    odd = rng.integers(30, 200, size=(45, 71), dtype=np.uint8)                # 3195 pixels: the generic kernels
    odd4 = odd[None, :, :, None]
    assert np.array_equal(pkg.histogram(stack, batch=2), ref_hist(stack)) and last(L) == HIST_TILED
    assert np.array_equal(pkg.histogram(odd), ref_hist(odd4)[0]) and last(L) == HIST_GENERIC
    assert np.array_equal(pkg.equalize_hist(stack, batch=2), ref_tone(stack, EQUALIZE)[0]) and last(L) == TABLES_TILED
    assert np.array_equal(pkg.equalize_hist(stack, "joint", batch=2), ref_tone(stack, EQUALIZE, joint=1)[0])
    luma = ref_preset(ref_tone(ref_preset(stack, "rgb2ycbcr"), EQUALIZE, mask=1)[0], "ycbcr2rgb")
    assert np.array_equal(pkg.equalize_hist(stack, "luma", batch=2), luma)
    assert np.array_equal(pkg.equalize_hist(odd), ref_tone(odd4, EQUALIZE)[0][0, :, :, 0]) and last(L) == TABLES_GENERIC
    q = int(np.floor(0.01 * 65536))
    assert np.array_equal(pkg.auto_levels(stack, 0.01, batch=2), ref_tone(stack, STRETCH, q, q, 1)[0])
    assert np.array_equal(pkg.auto_levels(stack, joint=False, batch=2), ref_tone(stack, STRETCH)[0])
    assert np.array_equal(pkg.auto_levels(odd), ref_tone(odd4, STRETCH, joint=1)[0][0, :, :, 0])
