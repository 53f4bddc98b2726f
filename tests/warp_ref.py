"""The affine warp of include/mi_blur.h ("Affine warp") restated in numpy int64 from the header's text, and nothing of
the product's (not a test module; tests/resample_harness.py launches the filter).  takes_tiled() restates the eligibility rule of the header
(the exact walk over the tiles included) and tile_geometry() the tiles of blur_warp_tiled_kernel.  ref_warp_band() gives
a band of output rows from the input rows it needs alone, for images too large to restate whole; EXTREME, narrow_cases()
and LIMIT_MAPS are the extreme shapes, one-chunk rows and maps at the header's limits that the GPU tests, the CPU-device
tests and tests/san_tile_bounds.cpp all walk."""
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


def band_rows(m, mode, h, wo, Y0, Y1):
    """(lo, hi): the input rows lo..hi (inclusive) that output rows [Y0, Y1) of a warp to `wo` columns need from an image
    of h rows.  An affine map has its extrema at the band's four corner pixels, so every first tap lies between their
    smallest and largest y0, every second tap at most one row further; both ends clamped into the image."""
    _, y0, _, _ = ref_coord(m, mode, [0, wo - 1, 0, wo - 1], [Y0, Y0, Y1 - 1, Y1 - 1])
    return int(np.clip(y0.min(), 0, h - 1)), int(np.clip(y0.max() + 1, 0, h - 1))


def ref_warp_band(rows, h, m, wo, Y0, Y1, mode=BILINEAR, border=CONSTANT, fill=0):
    """Output rows [Y0, Y1) of ref_warp(img, m, wo, Ho >= Y1, ...) for an image of h rows, from the slab of input rows
    band_rows() names alone: rows(lo, hi) returns input rows lo..hi - 1 as N x (hi - lo) x W x C.  The band is the warp of
    the slab under m moved by Y0 output rows and lo input rows.  A tap misses the slab only where it misses the image on
    the same side (the slab ends inside the image only beyond the band's last tap), so CLAMP repeats the image's own edge
    row and CONSTANT fills the same taps."""
    lo, hi = band_rows(m, mode, h, wo, Y0, Y1)
    slab = rows(lo, hi + 1)
    assert slab.shape[1] == hi - lo + 1
    mb = list(m)
    mb[2] += m[1] * Y0
    mb[5] += m[4] * Y0 - lo * Q
    return ref_warp(slab, mb, wo, Y1 - Y0, mode, border, fill)


def outside_share(m, mode, w, h, wo, Y0, Y1):
    """The share of output pixels of rows [Y0, Y1) none of whose taps lies inside the W x H image: `fill` under CONSTANT."""
    Y, X = np.mgrid[Y0:Y1, 0:wo].astype(np.int64)
    x0, y0, _, _ = ref_coord(m, mode, X, Y)
    k = 0 if mode == NEAREST else 1
    return float(((x0 + k < 0) | (x0 > w - 1) | (y0 + k < 0) | (y0 > h - 1)).mean())


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


# ---------------------------------------------------------------- cases the GPU tests, the CPU-device tests and
# tests/san_tile_bounds.cpp share
# Extreme shapes: ((input h, w, c), (Wo, Ho), m, k where the map is np.rot90(img, k) exactly).  All take the tiled kernel
# under both borders; positions (Q16) reach 2^31 along the 32768-long axis (the last two pass it).
EXTREME = [((1, 32768, 1), (32768, 1), [Q, 0, 3 * Q // 8 + 1, 0, Q, 0], None),                 # one row, 512 strips
           ((2, 32768, 1), (16384, 2), [2 * Q, 0, Q // 2, 0, Q, Q // 3], None),                # 2x reduction: sx passes 2^31
           ((32768, 16, 1), (16, 32768), rotation_m(16, 32768, 0.02), None),                   # 1024 tile rows of one chunk per row
           ((16, 32768, 1), (16, 32768), rot90_matrix(32768), 1),                              # m[2] = 2^31 - 2^16: columns become rows
           ((32768, 16, 1), (32768, 16), [0, Q, 0, -Q, 0, 32767 * Q], 3),                      # the transpose back
           ((3, 16384, 4), (32768, 3), [Q // 2, 0, -Q // 4, 0, Q, 0], None),                   # 8192 output chunks per row
           ((2, 32768, 3), (32768, 2), [Q, 0, -5 * Q // 8, 0, Q, Q // 2], None),               # 2048 groups of three chunks
           # the cases above stay just below 2^31; these two pass it by 40 pixels, beyond the right and the bottom edge, where a
           # position kept in 32 bits wraps to the opposite edge (what CLAMP repeats tells them apart)
           ((2, 32768, 1), (16384, 2), [2 * Q, 0, 40 * Q + Q // 2, 0, Q, Q // 3], None),
           ((32768, 16, 1), (16, 32768), [Q, 0, Q // 3, 0, Q, 40 * Q + Q // 2], None)]


def extreme_id(case):
    return "x".join(map(str, case[0])) + f"-{case[1][0]}x{case[1][1]}-at{case[2][2] >> 16},{case[2][5] >> 16}"       # input, output, the pixel output (0, 0) reads


def corner_pixels(wo, ho):
    return [(0, 0), (wo - 1, 0), (0, ho - 1), (wo - 1, ho - 1)]


# (input shape, (Wo, Ho)) of the warp, perspective and remap tests: 144 x 70 pixels out of 96 x 80 for one channel is
# 9 chunks x 70 rows = 3 x 3 tiles; the others likewise span more than one tile both ways, with output sizes that differ from the input's
TILED_SHAPES = [((1, 80, 96, 1), (144, 70)), ((2, 80, 96, 2), (136, 70)), ((1, 80, 96, 3), (144, 70)), ((2, 80, 96, 4), (132, 70))]


def edge_image(rng, n, h, w, c):
    """Noise, with 0 / 255 on the outermost rows and columns of image 0 (what CLAMP repeats and CONSTANT blends with the
    fill) and an all-255 last image when there are two."""
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    img[0, 0], img[0, -1], img[0, :, 0], img[0, :, -1] = 255, 0, 0, 255
    if n > 1:
        img[-1] = 255
    return img


# Inputs of one 16-byte chunk per row (3 channels: one group of three chunks): the staged box of the tiled kernel is the whole row, or the whole image.
NARROW_ROWS = [(16, 1), (8, 2), (16, 3), (4, 4)]        # (w, c)
NARROW_HEIGHTS = (1, 2, 33)
NARROW_N = 2


def impulse_rows(rng, n, h, w, c):
    """N x h x w x c random bytes with 0 / 255 impulses in the first and the last pixel of every row."""
    img = rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8)
    flip = (np.arange(n)[:, None] + np.arange(h)[None, :]) % 2 == 1
    img[:, :, 0, :] = np.where(flip, 255, 0)[:, :, None]
    img[:, :, -1, :] = np.where(flip, 0, 255)[:, :, None]
    return img


def narrow_cases():
    """(img, name, m, Wo, Ho): three 64-pixel strips and two tile rows out of every one-chunk row; an enlargement, a
    rotation, a sub-pixel shift and a map that lies wholly left of the image."""
    rng = np.random.default_rng(78)
    for w, c in NARROW_ROWS:
        assert w * c == (48 if c == 3 else 16)              # one chunk; for 3 channels one group of three
        wo, ho = (132 if c == 4 else 144), 33
        for h in NARROW_HEIGHTS:
            img = impulse_rows(rng, NARROW_N, h, w, c)
            for name, m in (("x4", scale_matrix(4, 1)), ("rot30", rotation_m(w, h, 30)), ("subpixel", [Q, 0, -3 * Q // 8, 0, Q, 5 * Q // 8]),
                            ("far-left", identity(-w - 3, 1))):
                yield img, name, m, wo, ho


# Maps at the limits of the header (linear part 2^26, translation 2^46) and degenerate maps, on a LIMIT_HW x LIMIT_HW input:
# name -> (m, class (classify()), for a wholly-outside map what CLAMP repeats (limit_clamp_want())).  The last two carry a
# limit coefficient and still put a whole output column, or row, inside the image.
LIMIT_HW = 64
_L, _O = LIN_MAX, OFF_MAX
LIMIT_MAPS = {
    "L-scale": ([_L, 0, 0, 0, _L, 0], "single", None),
    "L-antidiagonal": ([-_L, _L, 63 * Q, _L, -_L, 63 * Q], "single", None),
    "L-last-pixel": ([_L, 0, -79 * _L + 5 * Q, 0, _L, -39 * _L + 7 * Q + 123], "single", None),          # only output (79, 39) lands in the image
    "O-far": ([Q, 0, _O, 0, Q, _O], "outside", "bottom-right"),
    "O-far-negative": ([-Q, 0, -_O, 0, -Q, -_O], "outside", "top-left"),
    "O-left": ([Q, 0, -_O, 0, Q, 3 * Q], "outside", "left-edge"),
    "L-O-all": ([_L, _L, _O, -_L, -_L, -_O], "outside", "top-right"),
    "zero-linear": ([0, 0, 10 * Q + 777, 0, 0, 20 * Q + 31111], "single", None),
    "rank-one": ([Q, 0, 0, Q, 0, Q // 3], "varied", None),
    "step-1/65536": ([1, 0, 5 * Q, 0, 1, 6 * Q + 65535], "single", None),
    "L-one-column": ([_L, 0, -40 * _L + 30 * Q, 0, Q, 0], "varied", None),
    "L-one-row": ([Q, 0, 0, _L, Q, -20 * _L], "varied", None),
}
LIMIT_INSIDE = ("L-one-column", "L-one-row")
LIMIT_FILL = 173


def limit_out(c):
    """80 x 40, or 96 x 40 for 3 channels: whole groups of three chunks."""
    return (96 if c == 3 else 80), 40


def limit_corners(n, c):
    """The corner bytes of limit_image(): top-left, top-right, bottom-left, bottom-right of image i are 1 + 4 i .. 4 + 4 i."""
    return [[1 + 4 * i, 2 + 4 * i, 3 + 4 * i, 4 + 4 * i] for i in range(n)]


def limit_image(n, c):
    """N x 64 x 64 x c: interior bytes 16..159, the four edges 200 / 210 (top / bottom rows) and 220 / 230 (left / right
    columns), four distinct corner bytes per image, none of them LIMIT_FILL: a clamp to the wrong side shows."""
    img = np.random.default_rng(64 + c).integers(16, 160, size=(n, LIMIT_HW, LIMIT_HW, c), dtype=np.uint8)
    img[:, 0], img[:, -1] = 200, 210
    img[:, 1:-1, 0], img[:, 1:-1, -1] = 220, 230
    for i, (tl, tr, bl, br) in enumerate(limit_corners(n, c)):
        img[i, 0, 0], img[i, 0, -1], img[i, -1, 0], img[i, -1, -1] = tl, tr, bl, br
    return img


def classify(m, mode, w, h, wo, ho):
    """"outside": no output pixel has a tap inside the image; "single": those that have one all share one first tap (x0, y0);
    "varied": they read more than one."""
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    x0, y0, _, _ = ref_coord(m, mode, X, Y)
    k = 0 if mode == NEAREST else 1
    inside = (x0 + k >= 0) & (x0 <= w - 1) & (y0 + k >= 0) & (y0 <= h - 1)
    firsts = set(zip(x0[inside].tolist(), y0[inside].tolist()))
    return "outside" if not firsts else "single" if len(firsts) == 1 else "varied"


def limit_clamp_want(img, what, wo, ho):
    """What CLAMP gives for a wholly-outside map of LIMIT_MAPS: one corner of each image, or rows 3.. of its left edge."""
    n, h, w, c = img.shape
    if what == "left-edge":
        return np.broadcast_to(img[:, 3:3 + ho, :1], (n, ho, wo, c))
    y, x = {"top-left": (0, 0), "top-right": (0, w - 1), "bottom-left": (h - 1, 0), "bottom-right": (h - 1, w - 1)}[what]
    return np.broadcast_to(img[:, y:y + 1, x:x + 1], (n, ho, wo, c))


def limit_references(n, c):
    """(img, {(name, mode, border): ref_warp}) for LIMIT_MAPS on limit_image(n, c).  Many of these outputs are nearly constant,
    which a kernel that writes only `fill` or only one corner would give too; so, on the reference alone: every map is of
    the class LIMIT_MAPS states; a wholly-outside map gives the stated corner or edge under CLAMP (and `fill` under
    CONSTANT); no two wholly-outside maps that repeat different parts of the image share an output; the maps of
    LIMIT_INSIDE put at least 30 output pixels inside the image that are neither `fill` nor a corner byte."""
    img = limit_image(n, c)
    wo, ho = limit_out(c)
    corner_bytes = [LIMIT_FILL] + sum(limit_corners(n, c), [])
    refs = {}
    for name, (m, cls, what) in LIMIT_MAPS.items():
        for mode in (BILINEAR, NEAREST):
            assert classify(m, mode, LIMIT_HW, LIMIT_HW, wo, ho) == cls, (name, mode)
            for border in (CLAMP, CONSTANT):
                ref = refs[name, mode, border] = ref_warp(img, m, wo, ho, mode, border, LIMIT_FILL)
                if cls == "outside":
                    assert np.array_equal(ref, limit_clamp_want(img, what, wo, ho) if border == CLAMP else np.full_like(ref, LIMIT_FILL)), (name, mode, border)
                if name in LIMIT_INSIDE:
                    assert (~np.isin(ref, corner_bytes)).all(axis=3).sum() >= 30 * n, (name, mode, border)
    outside = [(name, what) for name, (_, cls, what) in LIMIT_MAPS.items() if cls == "outside"]
    assert len({what for _, what in outside}) == len(outside) == 4
    for mode in (BILINEAR, NEAREST):
        for i, (a, _) in enumerate(outside):
            for b, _ in outside[i + 1:]:
                assert not np.array_equal(refs[a, mode, CLAMP], refs[b, mode, CLAMP]), (a, b, mode)
    return img, refs


def make_warp(pkg, m, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0):
    return pkg.Warp(wo, ho, mode, border, fill, (C.c_int64 * 6)(*[int(v) for v in m]))
