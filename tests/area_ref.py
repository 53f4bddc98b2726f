"""The area resize of include/mi_blur.h ("Area resize") restated in numpy int64 from the header's text, and nothing of the
product's (not a test module; tests/resample_harness.py launches the filter through AREA, the family's Resampler).
takes_tiled() mirrors the eligibility rule of the header, and tile_geometry() restates the tiles of
blur_area_tiled_kernel for placing seams.  A spec is (wo, ho)."""
import numpy as np

from resample_harness import Resampler

MAX_DIM = 32768
MAX_RATIO = 64
# blur_area_tiled_kernel's tile (area_kernels.hip; AREA_TH / AREA_WAVE_SPAN of filter.h): TILE_ROWS OUTPUT rows x a strip of
# OUTPUT 16-byte chunk columns in whole units (3 chunks for 3 channels, else 1), cut so that the input chunks under a strip
# number at most WAVE_SPAN where one unit allows it
TILE_ROWS, WAVE_SPAN = 4, 64


def ref_weights(n_in, n_out):
    """The (n_out, n_in) int64 matrix w(X, i), word for word from the header: the overlap of output X's interval
    [X n_in, (X+1) n_in) with input i's [i n_out, (i+1) n_out), 0 where they do not meet."""
    X = np.arange(n_out, dtype=np.int64)[:, None]
    i = np.arange(n_in, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((X + 1) * n_in, (i + 1) * n_out) - np.maximum(X * n_in, i * n_out), 0)


def ref_axis(n_in, n_out):
    """(i_lo, i_hi, w_lo, w_hi) int64 arrays over X = 0 .. n_out - 1 in the form mi_blur_area_coord reports them, from the
    header's two floors and its w(X, i), without the weight matrix (32768 -> 512 would be 16 M entries)."""
    X = np.arange(n_out, dtype=np.int64)
    i_lo = (X * n_in) // n_out
    i_hi = ((X + 1) * n_in - 1) // n_out
    w = lambda i: np.minimum((X + 1) * n_in, (i + 1) * n_out) - np.maximum(X * n_in, i * n_out)
    return i_lo, i_hi, w(i_lo), np.where(i_hi > i_lo, w(i_hi), 0)


def ref_area(img, wo, ho):
    """img (N, H, W, C) uint8 -> (N, ho, wo, C) uint8."""
    n, h, w, c = img.shape
    wx, wy = ref_weights(w, wo), ref_weights(h, ho)
    s = np.einsum("yj,njic,xi->nyxc", wy, img.astype(np.int64), wx, optimize=True)
    d = w * h
    assert s.max(initial=0) <= 255 * d
    return ((2 * s + d) // (2 * d)).astype(np.uint8)


def prefix_sums(v, axis, n_in, n_out, X0, X1, first=0):
    """The weighted sums of outputs X0 .. X1 - 1 along `axis` of the int64 array v, which holds inputs first, first + 1, ...
    of n_in along that axis, from prefix sums and without a weight matrix: over the n_in * n_out fine units of the axis,
    P(t) = n_out * cum[t // n_out] + (t mod n_out) * v[t // n_out], and output X sums P((X + 1) n_in) - P(X n_in)."""
    v = np.moveaxis(v, axis, 0)
    cum = np.concatenate([np.zeros_like(v[:1]), np.cumsum(v, axis=0)])
    pad = np.concatenate([v, np.zeros_like(v[:1])])                       # P(n_in * n_out) reads one past the end, times 0
    t = np.arange(X0, X1 + 1, dtype=np.int64) * n_in
    k, r = t // n_out - first, t % n_out
    assert k.min() >= 0 and k.max() <= v.shape[0] and (k[r > 0] < v.shape[0]).all()
    P = n_out * cum[k] + r.reshape((-1,) + (1,) * (v.ndim - 1)) * pad[k]
    return np.moveaxis(np.diff(P, axis=0), 0, axis)


def ref_area_rows(slab, first_row, h, wo, ho, rows):
    """Output rows rows[0] .. rows[1] - 1 of ref_area for an image of h rows, of which slab (N, ., W, C) holds the rows from
    first_row on: at least the input rows i_lo(rows[0]) .. i_hi(rows[1] - 1) of ref_axis(h, ho).  int64 prefix sums, so it
    works at 32768 columns, where ref_weights() would not fit."""
    w = slab.shape[2]
    s = prefix_sums(slab.astype(np.int64), 1, h, ho, rows[0], rows[1], first_row)
    s = prefix_sums(s, 2, w, wo, 0, wo)
    d = w * h
    assert s.min(initial=0) >= 0 and s.max(initial=0) <= 255 * d
    return ((2 * s + d) // (2 * d)).astype(np.uint8)


def float_area(img, wo, ho):
    """The real-valued box average in float64, not rounded."""
    n, h, w, c = img.shape
    return np.einsum("yj,njic,xi->nyxc", ref_weights(h, ho) / float(h), img.astype(np.float64), ref_weights(w, wo) / float(w), optimize=True)


def valid(shape, wo, ho):
    n, h, w, c = shape
    return 1 <= wo <= MAX_DIM and 1 <= ho <= MAX_DIM and w <= MAX_RATIO * wo and h <= MAX_RATIO * ho


def takes_tiled(shape, wo, ho, offset_in=0, offset_out=0):
    """The header's rule for blur_area_tiled_kernel (dense strides: images W*H*C and Wo*Ho*C bytes apart)."""
    n, h, w, c = shape
    return (1 <= c <= 4 and wo <= w and ho <= h and (w * c) % 16 == 0 and (wo * c) % 16 == 0 and
            offset_in % 16 == 0 and offset_out % 16 == 0 and (w * h * c) % 16 == 0 and (wo * ho * c) % 16 == 0)


def strip_span(w, wo, c, x0c, nc):
    """The input chunks under output chunks [x0c, x0c + nc): first tap of their first pixel to last tap of their last."""
    x_lo, x_hi = (x0c * 16) // c, ((x0c + nc) * 16 - 1) // c
    i_lo, i_hi = (x_lo * w) // wo, ((x_hi + 1) * w - 1) // wo
    return (i_lo * c) // 16, (i_hi * c + c - 1) // 16


def tile_geometry(w, wo, ho, c):
    """(output chunk columns per strip, output chunk columns per row, output rows per tile, threads per row group) of the
    tiled kernel: strips of whole units, as wide as keeps every strip's span within WAVE_SPAN (at least one unit) and the
    last 64-dword step of a strip's output row at least half full (or the row within one step); the group is the power of
    two from 64 that holds the widest span."""
    cpr, unit = wo * c // 16, 3 if c == 3 else 1
    units = cpr // unit
    m = min(max((WAVE_SPAN - 3) * wo // (w * unit), 1), units)
    while True:
        nstrips = -(-units // m)
        ncols = unit * -(-units // nstrips)
        spans = [strip_span(w, wo, c, s * ncols, min(ncols, cpr - s * ncols)) for s in range(nstrips)]
        widest = max(hi - lo + 1 for lo, hi in spans)
        dwords = ncols * 4
        if m == 1 or (widest <= WAVE_SPAN and (dwords <= WAVE_SPAN or 2 * ((dwords - 1) % WAVE_SPAN + 1) >= WAVE_SPAN)):
            break
        m -= 1
    return ncols, cpr, TILE_ROWS, 64 if widest <= 64 else 128 if widest <= 128 else 256


def blocks(n, w, wo, ho, c):
    """Workgroups of a tiled launch."""
    ncols, cpr, rows, _ = tile_geometry(w, wo, ho, c)
    return n * -(-cpr // ncols) * -(-ho // rows)


AREA = Resampler(
    "area", "blur_area_tiled_kernel", "blur_area_generic_kernel",
    structs=lambda pkg, s: (pkg.Area(*s),),
    out_size=lambda s, w, h: (s[0], s[1]),
    set=lambda ctx, pkg, s: ctx.set_area(*s),
    ref=lambda img, s: ref_area(img, *s),
    takes_tiled=lambda shape, s, oi=0, oo=0: takes_tiled(shape, *s, oi, oo))
