"""What the colour transform's test files share (tests/test_color_{gpu,host}.py; not a test module, and not a conftest):
one launch through the C ABI inside guard bytes, on the GPU and on the CPU device.  resample_harness.py's Resampler
assumes an output with the input's channel count, which this filter does not have."""
import ctypes as C

import numpy as np


def make_color(pkg, m, bias, shift, lut=None, lut_on=None):
    """A pkg.Color from m (Co x up to 4), bias (Co), shift and lut (None or Co x 256).  lut_on: the field itself, where
    it shall differ from `lut is not None`."""
    m = np.asarray(m, np.int64)
    k = pkg.Color()
    k.out_channels, k.shift = m.shape[0], shift
    for o in range(m.shape[0]):
        for i in range(m.shape[1]):
            k.m[o][i] = int(m[o, i])
        k.bias[o] = int(bias[o])
    if lut is not None:
        t = np.ascontiguousarray(lut, dtype=np.uint8)
        for o in range(t.shape[0]):
            C.memmove(k.lut[o], t[o].ctypes.data, 256)
    k.lut_on = int(lut is not None) if lut_on is None else lut_on
    return k


def preset_color(pkg, L, name):
    k = pkg.Color()
    assert L.mi_blur_color_preset(pkg.COLOR_CODES[name], C.byref(k)) == pkg.OK
    return k


def gpu_run(pkg, L, torch, host, k, offset_in=0, offset_out=0):
    """host: N x H x W x C -> mi_blur_enqueue_color with the Color k.  The input lies offset_in bytes into a buffer with 64
    spare bytes, the output offset_out bytes into one with 128 bytes of 0x5A to spare: guards either side."""
    n, h, w, c = host.shape
    co = k.out_channels
    size_out = n * h * w * co
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    assert d_in.data_ptr() % 16 == 0 and d_out.data_ptr() % 16 == 0
    rc = L.mi_blur_enqueue_color(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, C.byref(k),
                                 torch.cuda.current_stream().cuda_stream)
    pkg.check(rc, "mi_blur_enqueue_color")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(n, h, w, co)


def cpu_run(pkg, L, img, k, n_threads, guard=256):
    """img: N x H x W x C -> mi_blur_cpu_run_color with the Color k.  The output starts as 0xA5 and the `guard` bytes before
    and after it must still hold 0xA5."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    size_out = n * h * w * k.out_channels
    buf = np.full(size_out + 2 * guard, 0xA5, np.uint8)
    pkg.check(L.mi_blur_cpu_run_color(a.ctypes.data, buf.ctypes.data + guard, w, h, c, n, C.byref(k), n_threads), "mi_blur_cpu_run_color")
    assert (buf[:guard] == 0xA5).all() and (buf[guard + size_out:] == 0xA5).all(), "wrote outside the output"
    return buf[guard:guard + size_out].reshape(n, h, w, k.out_channels)
