"""The distance transform restated from the definition in include/mi_blur.h ("Exact distance transform"), independent of
the product: the definition itself by brute force over all sites (small images), a separable numpy form (column
distances, then per row the W x W candidate matrix) for larger ones, and the limit and the byte forms in Python / numpy
integers.  Also the kernels' constants and routing rule for the shape lists (not a test module)."""
import numpy as np

L2, L1, LINF = 0, 1, 2
METRICS = (L2, L1, LINF)
NAMES = {L2: "l2", L1: "l1", LINF: "linf"}
BYTE, WITHIN = 0, 1
NONE = 0xFFFFFFFF
MAX_LIMIT = 32767
BAND = 32                   # rows per band of the column pass: DIST_BAND of csrc/filter.h
CHUNK = 16                  # columns per search chunk: 1 << DIST_CHUNK_LOG2
MAX_ROW = 24576             # the widest row (W * C) of the tiled kernel: DIST_MAX_ROW
TILE_ELEMS, MAX_ROWS = 4096, 8
TILED, GENERIC = "blur_dist_tiled_kernel", "blur_dist_generic_kernel"
BIG = np.int64(1) << 40     # "no site" inside the int64 arithmetic


def sites_of(img, nonzero=0):
    return (img != 0) if nonzero else (img == 0)


def combine(metric, dx, dy):
    """The metric of an offset, on integers or int64 arrays."""
    if metric == L2:
        return dx * dx + dy * dy
    if metric == L1:
        return dx + dy
    return np.maximum(dx, dy)


def apply_limit(metric, T, limit):
    """T (int64, BIG where there is no site) -> uint32 with NONE where there is no site or the distance exceeds the limit."""
    bound = combine(metric, np.int64(limit), np.int64(0)) if limit else BIG - 1
    return np.where(T <= bound, T, NONE).astype(np.uint32)


def ref_brute(img, metric, nonzero=0, limit=0):
    """The definition: img N x H x W x C uint8 -> uint32, the minimum over every site of the same image and channel."""
    n, h, w, c = img.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.int64)
    out = np.empty(img.shape, np.uint32)
    for i in range(n):
        for ch in range(c):
            sy, sx = np.nonzero(sites_of(img[i, :, :, ch], nonzero))
            if sy.size == 0:
                out[i, :, :, ch] = NONE
                continue
            d = combine(metric, np.abs(xs[:, :, None] - sx[None, None, :]), np.abs(ys[:, :, None] - sy[None, None, :]))
            out[i, :, :, ch] = apply_limit(metric, d.min(axis=2), limit)
    return out


def column_distance(site):
    """site: bool (..., H, W...) with rows on axis 1 of N x H x W x C -> int64 distance along the column to the nearest
    site of that column, BIG where the column has none."""
    n, h, w, c = site.shape
    rows = np.arange(h, dtype=np.int64).reshape(1, h, 1, 1)
    above = np.maximum.accumulate(np.where(site, rows, -BIG), axis=1)                    # the last site row at or above
    below = np.minimum.accumulate(np.where(site, rows, BIG)[:, ::-1], axis=1)[:, ::-1]    # the first at or below
    return np.minimum(np.where(above < 0, BIG, rows - above), np.where(below >= BIG, BIG, below - rows))


def ref_separable(img, metric, nonzero=0, limit=0):
    """The two passes in numpy: g down the columns, then per row the W x W matrix of candidates and its minimum."""
    n, h, w, c = img.shape
    g = column_distance(sites_of(img, nonzero))
    dx = np.abs(np.arange(w, dtype=np.int64)[:, None] - np.arange(w, dtype=np.int64)[None, :])      # [x, x']
    out = np.empty(img.shape, np.uint32)
    for i in range(n):
        for y in range(h):
            gy = g[i, y]                                                                  # [x', c]
            cand = np.where(gy[None] >= BIG, BIG, combine(metric, dx[:, :, None], np.where(gy >= BIG, 0, gy)[None]))
            out[i, y] = apply_limit(metric, cand.min(axis=1), limit)
    return out


def root_half_up(T):
    """The largest s with s == 0 or (2 s - 1)^2 <= 4 T, in Python integers."""
    T = int(T)
    s = 0
    while (2 * s + 1) ** 2 <= 4 * T:
        s += 1
    return s


def ref_value(metric, byte_op, invert, T, limit=0):
    """The byte for one table value, Python integers."""
    T = int(T)
    if byte_op == WITHIN:
        return 255 if (T != NONE) != bool(invert) else 0
    if T == NONE:
        return 255
    if metric == L2:
        return 255 if T >= 64771 else min(255, root_half_up(T))
    return min(255, T)


def ref_bytes(table, metric, byte_op=BYTE, invert=0):
    """A whole table -> uint8 (numpy; the root from the integer square root of 4 T, the float estimate corrected exactly)."""
    t = table.astype(np.int64)
    none = table == NONE
    if byte_op == WITHIN:
        return np.where(none != bool(invert), 0, 255).astype(np.uint8)
    if metric == L2:                                   # (2 s - 1)^2 <= 4 T  <=>  2 s - 1 <= isqrt(4 T)  <=>  s <= (isqrt(4 T) + 1) / 2
        r = np.floor(np.sqrt((4 * t).astype(np.float64))).astype(np.int64)
        r -= r * r > 4 * t
        r += (r + 1) * (r + 1) <= 4 * t
        out = np.minimum((r + 1) // 2, 255)
    else:
        out = np.minimum(t, 255)
    return np.where(none, 255, out).astype(np.uint8)


def takes_tiled(shape, offset_out=0):
    """The header's rule for blur_dist_tiled_kernel: W * C a multiple of 8, at most MAX_ROW, an aligned output."""
    n, h, w, c = shape
    return (w * c) % 8 == 0 and w * c <= MAX_ROW and offset_out % 16 == 0


def rows_per_group(shape):
    n, h, w, c = shape
    return max(1, min(MAX_ROWS, TILE_ELEMS // (w * c)))


def work_bytes(shape, band=BAND):
    n, h, w, c = shape
    return (n * h * w * c * 2 + 15) // 16 * 16 + n * -(-h // band) * 2 * w * c * 2
