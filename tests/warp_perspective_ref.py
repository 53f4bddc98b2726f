"""The perspective warp of include/mi_blur.h ("Perspective warp") restated in numpy int64 from the header's text (`//`
floors), with the setter's normalisation in float64, and nothing of the product's (not a test module).  It shares the
tile geometry and the limit image of warp_ref.py.  footprint() / max_footprint() / takes_tiled()
restate the eligibility rule with the corner rule; named_maps(), LIMIT_MAPS and EXTREME are the cases the host tests, the
GPU tests and tests/san_warp_perspective.cpp walk."""
import ctypes as C
import math

import numpy as np

from warp_ref import (BILINEAR, CLAMP, CONSTANT, LDS_MAX, LIMIT_FILL, LIMIT_HW, MAX_DIM, NEAREST, Q, limit_corners, limit_image, limit_out,
                      rotation_m, tile_geometry)

LIN_MAX, OFF_MAX = 1 << 32, 1 << 48
LIMITS = [LIN_MAX, LIN_MAX, OFF_MAX] * 3
MAX_K = 30


def affine_h(m, s=1):
    """The homography of the Q16 affine matrix m, scaled by s."""
    return [s * int(v) for v in m] + [0, 0, s * Q]


def position(h, X, Y):
    X, Y = np.asarray(X, dtype=np.int64), np.asarray(Y, dtype=np.int64)
    return h[0] * X + h[1] * Y + h[2], h[3] * X + h[4] * Y + h[5], h[6] * X + h[7] * Y + h[8]


def valid(h, wo, ho):
    """The header's limits and D >= 1 at the four corner pixels of the output."""
    if not (1 <= wo <= MAX_DIM and 1 <= ho <= MAX_DIM) or any(abs(int(v)) > lim for v, lim in zip(h, LIMITS)):
        return False
    return all(int(h[6]) * X + int(h[7]) * Y + int(h[8]) >= 1 for X in (0, wo - 1) for Y in (0, ho - 1))


def ref_coord(h, mode, X, Y):
    """(x0, y0, fx, fy), unclamped, for int64 arrays (or ints) X, Y: word for word from the header."""
    h = [int(v) for v in h]
    nx, ny, d = position(h, X, Y)
    assert (d >= 1).all()
    if mode == NEAREST:
        return (2 * nx + d) // (2 * d), (2 * ny + d) // (2 * d), np.zeros_like(nx), np.zeros_like(ny)
    px, py = (nx * 4096 + d) // (2 * d), (ny * 4096 + d) // (2 * d)
    return px >> 11, py >> 11, px & 2047, py & 2047


def ref_warp(img, h, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0):
    """img (N, H, W, C) uint8 -> (N, ho, wo, C) uint8.  px is clamped into [-2 * 2048, (W + 1) * 2048] before the split, as
    the header says implementations do."""
    n, hh, w, c = img.shape
    assert valid(h, wo, ho)
    h = [int(v) for v in h]
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    nx, ny, d = position(h, X, Y)
    if mode == NEAREST:
        x0, y0 = np.clip((2 * nx + d) // (2 * d), -2, w + 1), np.clip((2 * ny + d) // (2 * d), -2, hh + 1)
        fx = fy = np.zeros_like(x0)
    else:
        px, py = np.clip((nx * 4096 + d) // (2 * d), -2 * 2048, (w + 1) * 2048), np.clip((ny * 4096 + d) // (2 * d), -2 * 2048, (hh + 1) * 2048)
        x0, y0, fx, fy = px >> 11, py >> 11, px & 2047, py & 2047
    v = img.astype(np.int64)

    def tap(y, x):
        got = v[:, np.clip(y, 0, hh - 1), np.clip(x, 0, w - 1)]                  # N x ho x wo x C
        if border == CONSTANT:
            inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= hh - 1)
            got = np.where(inside[None, :, :, None], got, fill)
        return got
    if mode == NEAREST:
        return tap(y0, x0).astype(np.uint8)
    fx, fy = fx[None, :, :, None], fy[None, :, :, None]
    s = (2048 - fy) * ((2048 - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + fy * ((2048 - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1))
    assert s.max(initial=0) <= 255 << 22
    return ((s + (1 << 21)) >> 22).astype(np.uint8)


def float_warp(img, h, wo, ho, border=CONSTANT, fill=0):
    """Real-valued bilinear at the rational position in float64, not rounded (the numerators and D are below 2^53 for the
    maps this is used with)."""
    n, hh, w, c = img.shape
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    nx, ny, d = position([int(v) for v in h], X, Y)
    sx, sy = nx.astype(np.float64) / d, ny.astype(np.float64) / d
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    tx, ty = (sx - x0)[None, :, :, None], (sy - y0)[None, :, :, None]
    v = img.astype(np.float64)

    def tap(y, x):
        got = v[:, np.clip(y, 0, hh - 1), np.clip(x, 0, w - 1)]
        if border == CONSTANT:
            inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= hh - 1)
            got = np.where(inside[None, :, :, None], got, float(fill))
        return got
    return (1 - ty) * ((1 - tx) * tap(y0, x0) + tx * tap(y0, x0 + 1)) + ty * ((1 - tx) * tap(y0 + 1, x0) + tx * tap(y0 + 1, x0 + 1))


# ---------------------------------------------------------------- the setter, in float64
def adjugate(H):
    H = [float(v) for v in H]
    return [H[4] * H[8] - H[5] * H[7], H[2] * H[7] - H[1] * H[8], H[1] * H[5] - H[2] * H[4],
            H[5] * H[6] - H[3] * H[8], H[0] * H[8] - H[2] * H[6], H[2] * H[3] - H[0] * H[5],
            H[3] * H[7] - H[4] * H[6], H[1] * H[6] - H[0] * H[7], H[0] * H[4] - H[1] * H[3]]


def determinant(H):
    H = [float(v) for v in H]
    return H[0] * (H[4] * H[8] - H[5] * H[7]) - H[1] * (H[3] * H[8] - H[5] * H[6]) + H[2] * (H[3] * H[7] - H[4] * H[6])


def normalised(H, inverse):
    """v = (inverse ? H : adj H) / its last entry, in float64; None where the header says INVALID."""
    H = [float(v) for v in H]
    if not all(math.isfinite(v) for v in H):
        return None
    if not inverse:
        det = determinant(H)
        if det == 0.0 or not math.isfinite(det):
            return None
        H = adjugate(H)
    if H[8] == 0.0 or not math.isfinite(H[8]):
        return None
    v = [x / H[8] for x in H]
    return v if all(math.isfinite(x) for x in v) else None


def fraction_bits(v):
    """The largest k in 0..30 with |v_i| * 2^k <= limit_i - 1 for all nine entries; None when there is none."""
    for k in range(MAX_K, -1, -1):
        if all(abs(x) * 2.0 ** k <= lim - 1 for x, lim in zip(v, LIMITS)):
            return k
    return None


def set_matrix(H, inverse, wo, ho):
    """(h, k) of mi_blur_warp_perspective_set_matrix for an output of wo x ho; None where it answers INVALID."""
    v = normalised(H, inverse)
    k = None if v is None else fraction_bits(v)
    if k is None:
        return None
    h = [int(math.floor(x * 2.0 ** k + 0.5)) for x in v]
    return (h, k) if valid(h, wo, ho) else None


def quad_forward(src, dst):
    """The forward matrix of getPerspectiveTransform (H[8] = 1) by numpy.linalg.solve of the 8 x 8 system."""
    A, b = [], []
    for (x, y), (u, v) in zip(src, dst):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    return list(np.linalg.solve(np.array(A, dtype=np.float64), np.array(b, dtype=np.float64))) + [1.0]


def out_corners(wo, ho):
    return [(0.0, 0.0), (wo - 1.0, 0.0), (wo - 1.0, ho - 1.0), (0.0, ho - 1.0)]


def quad_h(w, h, wo, ho, quad):
    """The homography that takes the corners of a wo x ho output (top-left, top-right, bottom-right, bottom-left) to the
    source quad, through the restated setter with the forward matrix.  w, h: the input's size (the quads are stated in it)."""
    got = set_matrix(quad_forward(quad, out_corners(wo, ho)), False, wo, ho)
    assert got is not None, quad
    return got[0]


NAMED = ("keystone", "tilt", "flip-tilt", "half-out", "steep", "outside", "affine")


def named_quads(w, h):
    W, H = float(w), float(h)
    tilt = [(0.1 * W, 0.3 * H), (0.9 * W, 0.05 * H), (0.95 * W, 0.9 * H), (0.3 * W, 0.8 * H)]
    return {"keystone": [(0.2 * W, 0.1 * H), (0.8 * W, 0.1 * H), (W - 1, H - 1), (0.0, H - 1)],
            "tilt": tilt,
            "flip-tilt": [tilt[1], tilt[0], tilt[3], tilt[2]],
            "half-out": [(-0.4 * W, -0.3 * H), (0.7 * W, 0.1 * H), (0.6 * W, 0.6 * H), (-0.2 * W, 0.9 * H)],
            "steep": [(0.45 * W, 0.1 * H), (0.55 * W, 0.1 * H), (W - 1, H - 1), (0.0, H - 1)],
            "outside": [(2 * W, 0.0), (3 * W, 0.1 * H), (3 * W, H), (2 * W, 0.9 * H)]}


def named_maps(w, h, wo, ho):
    """name -> h for a W x H input and a Wo x Ho output."""
    out = {name: quad_h(w, h, wo, ho, quad) for name, quad in named_quads(w, h).items()}
    out["affine"] = affine_h(rotation_m(w, h, 30))
    assert tuple(out) == NAMED
    return out


# ---------------------------------------------------------------- the eligibility rule of the tiled kernel
def box(h, border, w, hh, X0, X1, Y0, Y1):
    """The input pixels (x0, x1, y0, y1) the tile of output pixels [X0, X1] x [Y0, Y1] stages: the box of the taps of its
    four corners with the + 1 tap, clamped into the image (CLAMP) or intersected with it (CONSTANT; None when empty)."""
    x0, y0, _, _ = ref_coord(h, BILINEAR, [X0, X1, X0, X1], [Y0, Y0, Y1, Y1])
    bx0, bx1, by0, by1 = int(x0.min()), int(x0.max()) + 1, int(y0.min()), int(y0.max()) + 1
    if border == CONSTANT:
        bx0, bx1, by0, by1 = max(bx0, 0), min(bx1, w - 1), max(by0, 0), min(by1, hh - 1)
        return None if bx0 > bx1 or by0 > by1 else (bx0, bx1, by0, by1)
    return min(max(bx0, 0), w - 1), min(max(bx1, 0), w - 1), min(max(by0, 0), hh - 1), min(max(by1, 0), hh - 1)


def footprint(h, border, w, hh, c, X0, X1, Y0, Y1):
    """Bytes of LDS of that tile, in whole 16-byte chunks; 0 when the box is empty."""
    b = box(h, border, w, hh, X0, X1, Y0, Y1)
    return 0 if b is None else (b[3] - b[2] + 1) * (((b[1] * c + c - 1) >> 4) - ((b[0] * c) >> 4) + 1) * 16


def tiles(wo, ho, c):
    """(X0, X1, Y0, Y1) of every tile of the output."""
    ncols, cpr, trows = tile_geometry(wo, ho, c)
    for ty0 in range(0, ho, trows):
        for x0c in range(0, cpr, ncols):
            nc = min(ncols, cpr - x0c)
            yield x0c * 16 // c, ((x0c + nc) * 16 - 1) // c, ty0, min(ty0 + trows, ho) - 1


def tile_footprints(shape, h, wo, ho, border):
    n, hh, w, c = shape
    return [footprint(h, border, w, hh, c, *t) for t in tiles(wo, ho, c)]


def max_footprint(shape, h, wo, ho, border):
    return max(tile_footprints(shape, h, wo, ho, border))


def takes_tiled(shape, h, wo, ho, mode=BILINEAR, border=CONSTANT, offset_in=0, offset_out=0):
    """The header's rule for blur_warp_persp_tiled_kernel (dense strides)."""
    n, hh, w, c = shape
    if not (mode == BILINEAR and 1 <= c <= 4 and (w * c) % 16 == 0 and (wo * c) % 16 == 0 and offset_in % 16 == 0 and
            offset_out % 16 == 0 and (w * hh * c) % 16 == 0 and (wo * ho * c) % 16 == 0):
        return False
    return max_footprint(shape, h, wo, ho, border) <= LDS_MAX


def outside_share(h, mode, w, hh, wo, ho):
    """The share of output pixels none of whose taps lies inside the W x H image."""
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    x0, y0, _, _ = ref_coord(h, mode, X, Y)
    k = 0 if mode == NEAREST else 1
    return float(((x0 + k < 0) | (x0 > w - 1) | (y0 + k < 0) | (y0 > hh - 1)).mean())


def classify(h, mode, w, hh, wo, ho):
    """warp_ref.classify() for a homography."""
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    x0, y0, _, _ = ref_coord(h, mode, X, Y)
    k = 0 if mode == NEAREST else 1
    inside = (x0 + k >= 0) & (x0 <= w - 1) & (y0 + k >= 0) & (y0 <= hh - 1)
    firsts = set(zip(x0[inside].tolist(), y0[inside].tolist()))
    return "outside" if not firsts else "single" if len(firsts) == 1 else "varied"


# ---------------------------------------------------------------- maps at the limits of the header, on warp_ref's 64 x 64
# limit_image and limit_out(c): name -> (h(Wo), class under BILINEAR, class under NEAREST, for a wholly-outside class the
# input pixel (x, y) CLAMP repeats)
_L, _O = LIN_MAX, OFF_MAX
LIMIT_MAPS = {
    "den-one": (lambda wo: [0, 0, 30 * wo, 0, 0, 20 * wo, -1, 0, wo], "varied", "varied", None),            # D = 1 in the last column
    "L-all": (lambda wo: [_L, 0, 10 * _O // 16, 0, _L, 5 * _O // 16, _L, _L, _O], "single", "single", None),
    "L-neg-den": (lambda wo: [_L, 0, 0, 0, _L, 0, -_L, -_L, 95 * _L + 39 * _L + 1], "varied", "varied", None),  # D = 1 at the last pixel when Wo = 96
    "O-over-O": (lambda wo: [0, 0, _O, 0, 0, -_O, 0, 0, _O], "single", "outside", (1, 0)),                  # the position (1, -1)
    "O-far": (lambda wo: [_L, 0, _O, 0, _L, _O, 0, 0, 1], "outside", "outside", (LIMIT_HW - 1, LIMIT_HW - 1)),   # quotients near 2^60
    "unit-den": (lambda wo: [3, 0, -7, 0, 2, 5, 0, 0, 1], "varied", "varied", None),
    "step-tiny": (lambda wo: [1, 0, 5 * _O // 64, 0, 1, 6 * _O // 64 + 12345, 0, 0, _O // 64], "single", "single", None),
    "den-grows": (lambda wo: [Q, 0, 0, 0, Q, 0, Q // 8, Q // 16, Q], "varied", "varied", None),
}


def limit_references(n, c):
    """(img, {(name, mode, border): ref_warp}) for LIMIT_MAPS on limit_image(n, c), with, on the reference alone: every map
    valid and of the stated class in each mode; a wholly-outside map gives the stated input pixel under CLAMP and `fill`
    under CONSTANT; every "varied" map has at least 30 output pixels per image that are neither `fill` nor a corner byte."""
    img = limit_image(n, c)
    wo, ho = limit_out(c)
    corner_bytes = [LIMIT_FILL] + sum(limit_corners(n, c), [])
    refs = {}
    for name, (hf, cls_b, cls_n, what) in LIMIT_MAPS.items():
        h = hf(wo)
        assert valid(h, wo, ho), name
        for mode, cls in ((BILINEAR, cls_b), (NEAREST, cls_n)):
            assert classify(h, mode, LIMIT_HW, LIMIT_HW, wo, ho) == cls, (name, mode)
            for border in (CLAMP, CONSTANT):
                ref = refs[name, mode, border] = ref_warp(img, h, wo, ho, mode, border, LIMIT_FILL)
                if cls == "outside":
                    want = np.broadcast_to(img[:, what[1]:what[1] + 1, what[0]:what[0] + 1], ref.shape) if border == CLAMP else np.full_like(ref, LIMIT_FILL)
                    assert np.array_equal(ref, want), (name, mode, border)
                if cls == "varied":
                    assert (~np.isin(ref, corner_bytes)).all(axis=3).sum() >= 30 * n, (name, mode, border)
    return img, refs


# Extreme shapes: ((input h, w, c), (Wo, Ho), h, border or None for both).  Both take the tiled kernel.
EXTREME = [((1, 32768, 1), (32768, 1), [1 << 30, 0, 0, 0, 1 << 30, 0, 1 << 14, 0, 1 << 30], None),        # one row, 512 strips; D doubles along it
           ((32768, 16, 1), (16, 32768), [1 << 30, 0, 0, 0, 1 << 30, 0, 0, -(1 << 13), 1 << 30], CLAMP)]   # one chunk wide; runs off the bottom

# A footprint over 64 KiB: the quad on a 512 x 512 x 1 input; to 64 x 64 it is generic, to 128 x 128 tiled
BIG_QUAD = [(100.0, 0.0), (411.0, 0.0), (511.0, 511.0), (0.0, 511.0)]


def make_persp(pkg, h, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0):
    return pkg.WarpPerspective(wo, ho, mode, border, fill, (C.c_int64 * 9)(*[int(v) for v in h]))
