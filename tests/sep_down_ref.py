"""The decimating separable filter of include/mi_blur.h restated in numpy — sep_ref.ref_sep, then the subsampling, and
nothing else — with the runners tests/test_sep_down_host.py and tests/test_sep_down_gpu.py share (not a test module).
The runners keep filter_harness's guards for an output that is smaller than the input: the input offset into a padded
buffer, the output surrounded by 0x5A (GPU) or prefilled with 0xA5 with a guard region after it (CPU)."""
import ctypes as C

import numpy as np

from sep_ref import ref_sep

PRESETS = {0: ([1, 4, 6, 4, 1], 2), 1: ([0, 1, 1], 2), 2: ([0, 0, 0, 1, 1, 1, 1], 4)}     # MI_BLUR_DOWN_*: taps of both axes, stride
PHASES = [(sx, sy, ox, oy) for sx in range(1, 5) for sy in range(1, 5) for ox in range(sx) for oy in range(sy)]


def ref_sep_down(img, wx, wy, sx=2, sy=2, ox=0, oy=0, rows=None, first_row=0):
    """img (N, H, W, C) uint8: the separable filter on the whole image, of which row oy + Y*sy and column ox + X*sx are kept.
    rows = (Y0, Y1): output rows Y0 .. Y1 - 1 only, from a slab: img then holds the image's rows from first_row on, and must
    hold the input rows of those outputs with len(wy) // 2 rows above and below as far as the image has them (where the
    slab ends at the image's edge, the padding is the image's own clamp)."""
    full = ref_sep(img, wx, wy)
    if rows is not None:
        first = oy + rows[0] * sy - first_row
        assert first >= 0 and first + (rows[1] - rows[0] - 1) * sy < img.shape[1]
        return np.ascontiguousarray(full[:, first:first + (rows[1] - rows[0] - 1) * sy + 1:sy, ox::sx, :])
    return np.ascontiguousarray(full[:, oy::sy, ox::sx, :])


def down_shape(shape, sx, sy, ox, oy):
    n, h, w, c = shape
    return n, (h - oy + sy - 1) // sy, (w - ox + sx - 1) // sx, c


def gpu_down_run(pkg, L, torch, host, kernel, dec, offset_in=0, offset_out=0):
    """host: N x H x W x C -> mi_blur_enqueue_sep_down with dec = (sx, sy, ox, oy).  The input lies offset_in bytes into a
    buffer with 64 spare bytes, the output offset_out bytes into one with 128 bytes of 0x5A to spare: guards either side."""
    n, h, w, c = host.shape
    oshape = down_shape(host.shape, *dec)
    size_out = int(np.prod(oshape))
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    d = pkg.Decimation(*dec)
    rc = L.mi_blur_enqueue_sep_down(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, C.byref(kernel), C.byref(d),
                                    torch.cuda.current_stream().cuda_stream)
    pkg.check(rc, "mi_blur_enqueue_sep_down")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(oshape)


def cpu_down_run(pkg, L, img, kernel, dec, n_threads, guard=256):
    """img: N x H x W x C -> mi_blur_cpu_run_sep_down.  The output starts as 0xA5, so a byte left unwritten shows, and the
    `guard` bytes after it must still hold 0xA5 afterwards."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    oshape = down_shape(a.shape, *dec)
    size_out = int(np.prod(oshape))
    buf = np.full(size_out + guard, 0xA5, np.uint8)
    d = pkg.Decimation(*dec)
    pkg.check(L.mi_blur_cpu_run_sep_down(a.ctypes.data, buf.ctypes.data, w, h, c, n, C.byref(kernel), C.byref(d), n_threads), "mi_blur_cpu_run_sep_down")
    assert (buf[size_out:] == 0xA5).all(), "wrote past the decimated output"
    return buf[:size_out].reshape(oshape)
