"""The affine warp of include/mi_blur.h ("Affine warp") restated in numpy int64 from the header's text, and nothing of
the product's — with the runners tests/test_warp_host.py and tests/test_warp_gpu.py share (not a test module).  The
runners keep resize_ref's guards: the input offset into a padded buffer, the output surrounded by 0x5A (GPU) or
prefilled with 0xA5 with a guard region either side (CPU).  takes_tiled() restates the eligibility rule of the header
(the exact walk over the tiles included) and tile_geometry() the tiles of blur_warp_tiled_kernel."""
import ctypes as C
import math

import numpy as np

NEAREST, BILINEAR = 0, 1
CLAMP, CONSTANT = 0, 1
MAX_DIM = 32768
Q = 1 << 16
LIN_MAX, OFF_MAX = 1 << 26, 1 << 46
# blur_warp_tiled_kernel's tile: TILE_ROWS OUTPUT rows x at most 4 * C OUTPUT 16-byte chunk columns (TILE_PX pixels); its
# footprint may take LDS_MAX bytes (64 KiB less 16)
TILE_ROWS, TILE_PX, LDS_MAX = 32, 64, 65520


def identity(shift_x=0, shift_y=0):
    """Output (X, Y) reads input (X + shift_x, Y + shift_y)."""
    return [Q, 0, shift_x * Q, 0, Q, shift_y * Q]


def rot90_matrix(w):
    """The header's m for np.rot90 of an image W wide: the output is H wide and W high."""
    return [0, -Q, (w - 1) * Q, Q, 0, 0]


def scale_matrix(num, den):
    """The header's m that equals the resize to num / den times the size under CLAMP: the map is OUTPUT -> INPUT, so its
    step is s = Q * den / num input pixels per output pixel, and t = (s - Q) / 2.  Both must be integers."""
    assert (Q * den) % num == 0
    s = Q * den // num
    assert (s - Q) % 2 == 0
    t = (s - Q) // 2
    return [s, 0, t, 0, s, t]


def rotation_forward(cx, cy, angle_deg, scale=1.0):
    """getRotationMatrix2D in float64, from the header's formula."""
    a, b = scale * math.cos(math.radians(angle_deg)), scale * math.sin(math.radians(angle_deg))
    return [a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy]


def invert(fwd):
    a, b, tx, c, d, ty = fwd
    det = a * d - b * c
    ia, ib, ic, id_ = d / det, -b / det, -c / det, a / det
    return [ia, ib, -(ia * tx + ib * ty), ic, id_, -(ic * tx + id_ * ty)]


def quantise(m):
    """q = floor(v * 65536 + 0.5)."""
    return [int(math.floor(v * 65536.0 + 0.5)) for v in m]


def rotation_m(w, h, angle_deg, scale=1.0, center=None):
    """The Q16 OUTPUT -> INPUT matrix of a rotation about the centre ((W-1)/2, (H-1)/2) by default."""
    cx, cy = center if center is not None else ((w - 1) / 2.0, (h - 1) / 2.0)
    return quantise(invert(rotation_forward(cx, cy, angle_deg, scale)))


def ref_coord(m, mode, X, Y):
    """(x0, y0, fx, fy), unclamped, for int64 arrays (or ints) X, Y: word for word from the header."""
    X, Y = np.asarray(X, dtype=np.int64), np.asarray(Y, dtype=np.int64)
    sx = m[0] * X + m[1] * Y + m[2]
    sy = m[3] * X + m[4] * Y + m[5]
    if mode == NEAREST:
        return (sx + 32768) >> 16, (sy + 32768) >> 16, np.zeros_like(sx), np.zeros_like(sy)
    px, py = (sx + 16) >> 5, (sy + 16) >> 5               # numpy's >> on int64 is arithmetic: it floors
    return px >> 11, py >> 11, px & 2047, py & 2047


def ref_warp(img, m, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0):
    """img (N, H, W, C) uint8 -> (N, ho, wo, C) uint8."""
    n, h, w, c = img.shape
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    x0, y0, fx, fy = ref_coord(m, mode, X, Y)
    v = img.astype(np.int64)

    def tap(y, x):
        got = v[:, np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]                  # N x ho x wo x C
        if border == CONSTANT:
            inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            got = np.where(inside[None, :, :, None], got, fill)
        return got
    if mode == NEAREST:
        return tap(y0, x0).astype(np.uint8)
    fx, fy = fx[None, :, :, None], fy[None, :, :, None]
    s = (2048 - fy) * ((2048 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + fy * ((2048 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1))
    assert s.max(initial=0) <= 255 << 22
    return ((s + (1 << 21)) >> 22).astype(np.uint8)


def float_warp(img, m, wo, ho, border=CONSTANT, fill=0):
    """Real-valued bilinear at the exact Q16 position in float64, not rounded."""
    n, h, w, c = img.shape
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    sx = (m[0] * X + m[1] * Y + m[2]).astype(np.float64) / Q
    sy = (m[3] * X + m[4] * Y + m[5]).astype(np.float64) / Q
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    tx, ty = (sx - x0)[None, :, :, None], (sy - y0)[None, :, :, None]
    v = img.astype(np.float64)

    def tap(y, x):
        got = v[:, np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        if border == CONSTANT:
            inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            got = np.where(inside[None, :, :, None], got, float(fill))
        return got
    return (1 - ty) * ((1 - tx) * tap(y0, x0) + tx * tap(y0, x0 + 1)) + ty * ((1 - tx) * tap(y0 + 1, x0) + tx * tap(y0 + 1, x0 + 1))


def tile_geometry(wo, ho, c):
    """(output chunk columns per strip, output chunk columns per row, output rows per tile) of the tiled kernel: the chunk
    columns of a row cut into ceil(cpr / (4 * C)) equal strips, for 3 channels of whole groups of 3 chunks (16 pixels)."""
    cpr = wo * c // 16
    unit = 3 if c == 3 else 1
    units, max_units = cpr // unit, (TILE_PX * c // 16) // unit
    nstrips = -(-units // max_units)
    return unit * -(-units // nstrips), cpr, TILE_ROWS


def footprint(m, border, w, h, c, X0, X1, Y0, Y1):
    """Bytes of LDS of the tile of output pixels [X0, X1] x [Y0, Y1]: the box of the taps of its four corners with the + 1
    tap, clamped into the image (CLAMP) or intersected with it (CONSTANT; 0 when empty), in whole 16-byte chunks."""
    x0, y0, _, _ = ref_coord(m, BILINEAR, [X0, X1, X0, X1], [Y0, Y0, Y1, Y1])
    bx0, bx1, by0, by1 = int(x0.min()), int(x0.max()) + 1, int(y0.min()), int(y0.max()) + 1
    if border == CONSTANT:
        bx0, bx1, by0, by1 = max(bx0, 0), min(bx1, w - 1), max(by0, 0), min(by1, h - 1)
        if bx0 > bx1 or by0 > by1:
            return 0
    else:
        bx0, bx1 = min(max(bx0, 0), w - 1), min(max(bx1, 0), w - 1)
        by0, by1 = min(max(by0, 0), h - 1), min(max(by1, 0), h - 1)
    return (by1 - by0 + 1) * (((bx1 * c + c - 1) >> 4) - ((bx0 * c) >> 4) + 1) * 16


def max_footprint(shape, m, wo, ho, border):
    n, h, w, c = shape
    ncols, cpr, trows = tile_geometry(wo, ho, c)
    worst = 0
    for ty0 in range(0, ho, trows):
        for x0c in range(0, cpr, ncols):
            nc = min(ncols, cpr - x0c)
            worst = max(worst, footprint(m, border, w, h, c, x0c * 16 // c, ((x0c + nc) * 16 - 1) // c, ty0, min(ty0 + trows, ho) - 1))
    return worst


def takes_tiled(shape, m, wo, ho, mode=BILINEAR, border=CONSTANT, offset_in=0, offset_out=0):
    """The header's rule for blur_warp_tiled_kernel (dense strides: images W*H*C and Wo*Ho*C bytes apart)."""
    n, h, w, c = shape
    if not (mode == BILINEAR and 1 <= c <= 4 and (w * c) % 16 == 0 and (wo * c) % 16 == 0 and offset_in % 16 == 0 and
            offset_out % 16 == 0 and (w * h * c) % 16 == 0 and (wo * ho * c) % 16 == 0):
        return False
    return max_footprint(shape, m, wo, ho, border) <= LDS_MAX


def in_the_admitted_region(m):
    """|m[0]| + |m[1]| <= 3Q/2 and |m[3]| + |m[4]| <= 3Q/2: every aligned BILINEAR launch in here takes the tiled kernel."""
    return abs(m[0]) + abs(m[1]) <= 3 * Q // 2 and abs(m[3]) + abs(m[4]) <= 3 * Q // 2


def make_warp(pkg, m, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0):
    return pkg.Warp(wo, ho, mode, border, fill, (C.c_int64 * 6)(*[int(v) for v in m]))


def gpu_warp_run(pkg, L, torch, host, m, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0, offset_in=0, offset_out=0):
    """host: N x H x W x C -> mi_blur_enqueue_warp.  The input lies offset_in bytes into a buffer with 64 spare bytes, the
    output offset_out bytes into one with 128 bytes of 0x5A to spare: guards either side."""
    n, h, w, c = host.shape
    oshape = (n, ho, wo, c)
    size_out = int(np.prod(oshape))
    d_in = torch.zeros(host.size + 64, dtype=torch.uint8, device="cuda")
    d_in[offset_in:offset_in + host.size] = torch.from_numpy(np.ascontiguousarray(host).reshape(-1)).cuda()
    d_out = torch.full((size_out + 128,), 0x5A, dtype=torch.uint8, device="cuda")
    wp = make_warp(pkg, m, wo, ho, mode, border, fill)
    rc = L.mi_blur_enqueue_warp(d_in.data_ptr() + offset_in, d_out.data_ptr() + offset_out, w, h, c, n, C.byref(wp),
                                torch.cuda.current_stream().cuda_stream)
    pkg.check(rc, "mi_blur_enqueue_warp")
    torch.cuda.synchronize()
    o = d_out.cpu().numpy()
    assert (o[:offset_out] == 0x5A).all() and (o[offset_out + size_out:] == 0x5A).all(), "wrote outside the output"
    return o[offset_out:offset_out + size_out].reshape(oshape)


def cpu_warp_run(pkg, L, img, m, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0, n_threads=2, guard=256):
    """img: N x H x W x C -> mi_blur_cpu_run_warp.  The output starts as 0xA5, so a byte left unwritten shows (the callers'
    images and fills avoid giving 0xA5 everywhere), and the `guard` bytes before and after it must still hold 0xA5."""
    a = np.ascontiguousarray(img)
    n, h, w, c = a.shape
    oshape = (n, ho, wo, c)
    size_out = int(np.prod(oshape))
    buf = np.full(size_out + 2 * guard, 0xA5, np.uint8)
    wp = make_warp(pkg, m, wo, ho, mode, border, fill)
    pkg.check(L.mi_blur_cpu_run_warp(a.ctypes.data, buf.ctypes.data + guard, w, h, c, n, C.byref(wp), n_threads), "mi_blur_cpu_run_warp")
    assert (buf[:guard] == 0xA5).all() and (buf[guard + size_out:] == 0xA5).all(), "wrote outside the warped output"
    return buf[guard:guard + size_out].reshape(oshape)
