"""The image resize of include/mi_blur.h ("Image resize") restated in numpy int64 from the header's text, and nothing of
the product's (not a test module; tests/resample_harness.py launches the filter).  takes_tiled() mirrors the eligibility
rule of the header, and tile_geometry() restates the tiles of blur_resize_tiled_kernel for placing seams."""
import numpy as np

NEAREST, BILINEAR = 0, 1
MAX_DIM = 32768
# blur_resize_tiled_kernel's tile (resize_kernels.hip; TILE_TH / TILE_NCOLS of kernel_common.h): TILE_ROWS OUTPUT rows x at
# most TILE_CHUNKS OUTPUT 16-byte chunk columns, the chunk columns of a row cut into equal strips
TILE_ROWS, TILE_CHUNKS = 32, 32


def ref_axis(n_in, n_out, mode=BILINEAR):
    """(a, b, f) int64 arrays over X = 0 .. n_out - 1, word for word from the header."""
    X = np.arange(n_out, dtype=np.int64)
    den = 2 * n_out
    if mode == NEAREST:
        i = ((2 * X + 1) * n_in) // den
        return i, i.copy(), np.zeros(n_out, np.int64)
    num = (2 * X + 1) * n_in - n_out
    i0 = num // den                                   # numpy's // floors towards minus infinity
    rem = num - i0 * den
    f = (rem * 2048 + n_out) // den
    return np.clip(i0, 0, n_in - 1), np.clip(i0 + 1, 0, n_in - 1), f


def ref_resize(img, wo, ho, mode=BILINEAR, rows=None, first_row=0, height=None):
    """img (N, H, W, C) uint8 -> (N, ho, wo, C) uint8.  rows = (Y0, Y1): output rows Y0 .. Y1 - 1 only, from a slab: img then
    holds the rows from first_row on of an image of `height` rows, and must hold the a and b rows of those outputs."""
    n, h, w, c = img.shape
    xa, xb, fx = ref_axis(w, wo, mode)
    ya, yb, fy = ref_axis(h if height is None else height, ho, mode)
    if rows is not None:
        ya, yb, fy = (v[rows[0]:rows[1]] for v in (ya - first_row, yb - first_row, fy))
        assert ya.min() >= 0 and yb.max() < h
    if mode == NEAREST:
        return np.ascontiguousarray(img[:, ya][:, :, xa])
    v = img.astype(np.int64)
    fx = fx[None, None, :, None]
    fy = fy[None, :, None, None]
    top = (2048 - fx) * v[:, ya][:, :, xa] + fx * v[:, ya][:, :, xb]
    bot = (2048 - fx) * v[:, yb][:, :, xa] + fx * v[:, yb][:, :, xb]
    s = (2048 - fy) * top + fy * bot
    assert s.max(initial=0) <= 255 << 22
    return ((s + (1 << 21)) >> 22).astype(np.uint8)


def float_bilinear(img, wo, ho):
    """Real-valued half-pixel bilinear in float64 (edges clamp), not rounded."""
    n, h, w, c = img.shape

    def axis(n_in, n_out):
        pos = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
        i0 = np.floor(pos)
        return np.clip(i0, 0, n_in - 1).astype(int), np.clip(i0 + 1, 0, n_in - 1).astype(int), pos - i0
    xa, xb, tx = axis(w, wo)
    ya, yb, ty = axis(h, ho)
    v = img.astype(np.float64)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    top = (1 - tx) * v[:, ya][:, :, xa] + tx * v[:, ya][:, :, xb]
    bot = (1 - tx) * v[:, yb][:, :, xa] + tx * v[:, yb][:, :, xb]
    return (1 - ty) * top + ty * bot


def takes_tiled(shape, wo, ho, mode=BILINEAR, offset_in=0, offset_out=0):
    """The header's rule for blur_resize_tiled_kernel (dense strides: images W*H*C and Wo*Ho*C bytes apart)."""
    n, h, w, c = shape
    return (mode == BILINEAR and 1 <= c <= 4 and wo >= w and ho >= h and (w * c) % 16 == 0 and (wo * c) % 16 == 0 and
            offset_in % 16 == 0 and offset_out % 16 == 0 and (w * h * c) % 16 == 0 and (wo * ho * c) % 16 == 0)


def tile_geometry(wo, ho, c):
    """(output chunk columns per strip, output chunk columns per row, output rows per tile) of the tiled kernel."""
    cpr = wo * c // 16
    nstrips = -(-cpr // TILE_CHUNKS)
    return -(-cpr // nstrips), cpr, TILE_ROWS
