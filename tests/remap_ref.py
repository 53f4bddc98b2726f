"""The remap of include/mi_blur.h ("Remap") restated in numpy int64 from the header's text, and nothing of the product's
-- with the box function and the tile walk of blur_remap_tiled_kernel restated (ref_box(), ref_plan()), the undistortion
formula in numpy float64 (ref_undistort()) and the maps tests/test_remap_host.py and tests/test_remap_gpu.py share (MAPS /
build_map()) (not a test module; tests/resample_harness.py launches the filter)."""
import numpy as np

import warp_perspective_ref as pr
import warp_ref as wr
from warp_ref import BILINEAR, CLAMP, CONSTANT, MAX_DIM, NEAREST, tile_geometry  # noqa: F401

FRAC, ONE = 11, 2048
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
STAGE_MAX = 65520                       # the default and the largest stage_bytes
QUANT_LIMIT = 1 << 30                   # mi_blur_remap_from_float clamps into +- this


# ---------------------------------------------------------------- the definition
def ref_coord(px, py, mode, w, h):
    """(x0, y0, fx, fy), clamped, for int64 arrays (or ints) px, py on a W x H image: word for word from the header."""
    out = []
    for v, n in ((px, w), (py, h)):
        p = np.clip(np.asarray(v, dtype=np.int64), -2 * ONE, (n + 1) * ONE)
        out.append(((p + 1024) >> FRAC, np.zeros_like(p)) if mode == NEAREST else (p >> FRAC, p & (ONE - 1)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def ref_remap(img, fmap, mode=BILINEAR, border=CONSTANT, fill=0):
    """img (N, H, W, C) uint8, fmap (Ho, Wo, 2) int32 -> (N, Ho, Wo, C) uint8."""
    n, h, w, c = img.shape
    x0, y0, fx, fy = ref_coord(fmap[:, :, 0], fmap[:, :, 1], mode, w, h)
    v = img.astype(np.int64)

    def tap(y, x):
        got = v[:, np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]                  # N x Ho x Wo x C
        if border == CONSTANT:
            inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            got = np.where(inside[None, :, :, None], got, fill)
        return got
    if mode == NEAREST:
        return tap(y0, x0).astype(np.uint8)
    fx, fy = fx[None, :, :, None], fy[None, :, :, None]
    s = (ONE - fy) * ((ONE - fx) * tap(y0, x0) + fx * tap(y0, x0 + 1)) + fy * ((ONE - fx) * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1))
    assert s.max(initial=0) <= 255 << 22
    return ((s + (1 << 21)) >> 22).astype(np.uint8)


def map_rows(fmap, mode, w, h):
    """(lo, hi): the input rows lo .. hi (inclusive) that the taps of fmap read from a W x H image, clamped into it."""
    _, y0, _, _ = ref_coord(fmap[:, :, 0], fmap[:, :, 1], mode, w, h)
    k = 0 if mode == NEAREST else 1
    return int(np.clip(y0.min(), 0, h - 1)), int(np.clip(y0.max() + k, 0, h - 1))


def ref_remap_slab(slab, first_row, h, fmap, mode=BILINEAR, border=CONSTANT, fill=0):
    """ref_remap of an image of h rows from the slab (N, ., W, C) of its rows from first_row on, which must hold the rows
    map_rows() names: the map's y entries, clamped as the image clamps them, shifted by first_row rows.  A tap misses the
    slab only where it misses the image on the same side, so where the slab ends at the image's edge the border is the
    image's own."""
    n, hs, w, c = slab.shape
    lo, hi = map_rows(fmap, mode, w, h)
    assert first_row <= lo and hi < first_row + hs and first_row + hs <= h
    shifted = np.asarray(fmap, dtype=np.int64).copy()
    shifted[:, :, 1] = np.clip(shifted[:, :, 1], -2 * ONE, (h + 1) * ONE) - first_row * ONE
    return ref_remap(slab, shifted, mode, border, fill)


def float_remap(img, xs, ys, border=CONSTANT, fill=0):
    """Real-valued bilinear at the real positions (xs, ys) (float64 (Ho, Wo) arrays), not rounded."""
    n, h, w, c = img.shape
    xs, ys = np.clip(xs, -2.0, w + 1.0), np.clip(ys, -2.0, h + 1.0)            # beyond: both taps outside on one side either way
    x0, y0 = np.floor(xs).astype(np.int64), np.floor(ys).astype(np.int64)
    tx, ty = (xs - x0)[None, :, :, None], (ys - y0)[None, :, :, None]
    v = img.astype(np.float64)

    def tap(y, x):
        got = v[:, np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)]
        if border == CONSTANT:
            inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            got = np.where(inside[None, :, :, None], got, float(fill))
        return got
    return (1 - ty) * ((1 - tx) * tap(y0, x0) + tx * tap(y0, x0 + 1)) + ty * ((1 - tx) * tap(y0 + 1, x0) + tx * tap(y0 + 1, x0 + 1))


def quantise(xs, ys):
    """mi_blur_remap_from_float: q = floor(v * 2048 + 0.5) in double, clamped into +-2^30; int32 (Ho, Wo, 2)."""
    q = [np.clip(np.floor(np.asarray(v, dtype=np.float64) * 2048.0 + 0.5), -QUANT_LIMIT, QUANT_LIMIT).astype(np.int64) for v in (xs, ys)]
    return np.stack(q, axis=-1).astype(np.int32)


def ref_undistort_real(K, dist, size, new_K=None):
    """The header's undistortion formula in float64, operation for operation: the real positions (u, v), each (Ho, Wo)."""
    fx, fy, cx, cy = (np.float64(v) for v in K)
    nfx, nfy, ncx, ncy = (np.float64(v) for v in (new_K if new_K is not None else K))
    k1, k2, p1, p2, k3 = (np.float64(v) for v in dist)
    wo, ho = size
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.float64)
    x, y = (X - ncx) / nfx, (Y - ncy) / nfy
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def ref_undistort(K, dist, size, new_K=None):
    return quantise(*ref_undistort_real(K, dist, size, new_K))


# ---------------------------------------------------------------- the tiled kernel's rule, box and walk
def shape_tiled(w, c, wo, mode=BILINEAR):
    """Eligible for blur_remap_tiled_kernel by shape."""
    return mode == BILINEAR and 1 <= c <= 4 and (w * c) % 16 == 0 and (wo * c) % 16 == 0


def takes_tiled(shape, wo, ho, mode=BILINEAR, offset_in=0, offset_out=0, offset_map=0):
    """The header's rule (dense strides): the affine tiled kernel's, plus a 16-byte aligned map."""
    n, h, w, c = shape
    return shape_tiled(w, c, wo, mode) and offset_in % 16 == 0 and offset_out % 16 == 0 and offset_map % 16 == 0


def ref_box(x0, y0, border, w, h):
    """(bx0, bx1, by0, by1) of a set of first taps, or None when empty: [min x0, max x0 + 1] x [min y0, max y0 + 1], clamped
    into the image (CLAMP) or intersected with it (CONSTANT)."""
    bx0, bx1, by0, by1 = int(x0.min()), int(x0.max()) + 1, int(y0.min()), int(y0.max()) + 1
    if border == CONSTANT:
        bx0, bx1, by0, by1 = max(bx0, 0), min(bx1, w - 1), max(by0, 0), min(by1, h - 1)
        return None if bx0 > bx1 or by0 > by1 else (bx0, bx1, by0, by1)
    cl = lambda v, n: min(max(v, 0), n - 1)
    return cl(bx0, w), cl(bx1, w), cl(by0, h), cl(by1, h)


def box_bytes(box, c):
    bx0, bx1, by0, by1 = box
    return (by1 - by0 + 1) * (((bx1 * c + c - 1) >> 4) - ((bx0 * c) >> 4) + 1) * 16


def ref_plan(fmap, w, h, c, mode=BILINEAR, border=CONSTANT, stage_bytes=0):
    """mi_blur_remap_plan restated: the walk over the warp kernel's tiles (tile_geometry()) of one output image."""
    ho, wo = fmap.shape[:2]
    out = dict(tiled=0, tiles=0, staged=0, direct=0, empty=0, max_box_bytes=0, max_staged_bytes=0)
    if not shape_tiled(w, c, wo, mode):
        return out
    stage = stage_bytes or STAGE_MAX
    out["tiled"] = 1
    x0, y0, _, _ = ref_coord(fmap[:, :, 0], fmap[:, :, 1], BILINEAR, w, h)
    ncols, cpr, trows = tile_geometry(wo, ho, c)
    for ty0 in range(0, ho, trows):
        for x0c in range(0, cpr, ncols):
            nc = min(ncols, cpr - x0c)
            X0, X1 = x0c * 16 // c, ((x0c + nc) * 16 - 1) // c
            sl = (slice(ty0, min(ty0 + trows, ho)), slice(X0, X1 + 1))
            box = ref_box(x0[sl], y0[sl], border, w, h)
            out["tiles"] += 1
            if box is None:
                out["empty"] += 1
                continue
            b = box_bytes(box, c)
            out["max_box_bytes"] = max(out["max_box_bytes"], b)
            if b <= stage:
                out["staged"] += 1
                out["max_staged_bytes"] = max(out["max_staged_bytes"], b)
            else:
                out["direct"] += 1
    return out


# ---------------------------------------------------------------- map builders: all int32 (Ho, Wo, 2)
def from_taps(x0, y0, fx, fy):
    """px = clip(x0 * 2048 + fx) into the int32 range, py likewise: the map that repeats a warp's coordinates."""
    px = np.clip(np.asarray(x0, dtype=np.int64) * ONE + fx, I32_MIN, I32_MAX)
    py = np.clip(np.asarray(y0, dtype=np.int64) * ONE + fy, I32_MIN, I32_MAX)
    return np.stack([px, py], axis=-1).astype(np.int32)


def identity_map(wo, ho, dx=0, dy=0):
    """Output (X, Y) reads the position (X, Y) + (dx, dy) / 2048."""
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    return np.stack([X * ONE + dx, Y * ONE + dy], axis=-1).astype(np.int32)


def affine_map(m, wo, ho):
    """The BILINEAR coordinates of the affine warp m (warp_ref.ref_coord: the restatement mi_blur_warp_coord is tested against)."""
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    return from_taps(*wr.ref_coord(m, BILINEAR, X, Y))


def perspective_map(hm, wo, ho):
    Y, X = np.mgrid[0:ho, 0:wo].astype(np.int64)
    return from_taps(*pr.ref_coord(hm, BILINEAR, X, Y))


def abi_affine_map(pkg, L, m, wo, ho):
    """The same through mi_blur_warp_coord itself, pixel by pixel."""
    wp = wr.make_warp(pkg, m, 1, 1, BILINEAR)
    out = np.empty((ho, wo, 2), np.int32)
    for Y in range(ho):
        for X in range(wo):
            x0, y0, fx, fy = pkg.warp_coord(wp, X, Y)
            out[Y, X] = (min(max(x0 * ONE + fx, I32_MIN), I32_MAX), min(max(y0 * ONE + fy, I32_MIN), I32_MAX))
    return out


def abi_perspective_map(pkg, L, hm, wo, ho):
    wp = pr.make_persp(pkg, hm, wo, ho, BILINEAR)
    out = np.empty((ho, wo, 2), np.int32)
    for Y in range(ho):
        for X in range(wo):
            x0, y0, fx, fy = pkg.warp_perspective_coord(wp, X, Y)
            out[Y, X] = (min(max(x0 * ONE + fx, I32_MIN), I32_MAX), min(max(y0 * ONE + fy, I32_MIN), I32_MAX))
    return out


BARREL_DIST = (-0.2, 0.05, 0.001, -0.002, 0.01)


def barrel_K(w, h):
    """The hosts' camera: fx = fy = W, the principal point at the image's centre."""
    return (float(w), float(w), (w - 1) / 2.0, (h - 1) / 2.0)


def barrel_map(w, h, wo, ho):
    """The undistortion map of the header's example coefficients; the new camera scales the old one to the output's size."""
    K = barrel_K(w, h)
    new_K = (K[0] * wo / w, K[1] * wo / w, (wo - 1) / 2.0, (ho - 1) / 2.0)
    return ref_undistort(K, BARREL_DIST, (wo, ho), new_K)


def extreme_entries(w):
    return [I32_MIN, I32_MAX, -4097, (w + 1) * ONE + 1]


def extremes_map(w, h, wo, ho):
    """The identity (scaled to the output's size) with the four extreme entries planted, in x, in y and in both, at tile
    corners (the warp kernel's tiles: 64 pixels x 32 rows) and in tile interiors."""
    m = identity_map(wo, ho)
    m[:, :, 0] = (m[:, :, 0].astype(np.int64) * w // wo).astype(np.int32)
    m[:, :, 1] = (m[:, :, 1].astype(np.int64) * h // ho).astype(np.int32)
    spots = [(0, 0), (wo - 1, 0), (0, ho - 1), (wo - 1, ho - 1), (min(63, wo - 1), min(31, ho - 1)), (min(64, wo - 1), min(32, ho - 1)),
             (wo // 2, ho // 2), (min(17, wo - 1), min(9, ho - 1)), (min(100, wo - 1), min(45, ho - 1)), (wo // 3, ho // 5), (2 * wo // 3, 4 * ho // 5), (wo // 5, ho // 3)]
    ex = extreme_entries(w)
    ey = [I32_MIN, I32_MAX, -4097, (h + 1) * ONE + 1]
    for i, (X, Y) in enumerate(spots):
        k = i % 4
        if i % 3 != 1:
            m[Y, X, 0] = ex[k]
        if i % 3 != 0:
            m[Y, X, 1] = ey[(k + i // 4) % 4]
    return m


MAPS = ("rot30", "barrel", "subpixel", "outside", "half-out", "wild", "extremes")      # every map but `mixed`, which has a shape of its own


def build_map(name, w, h, wo, ho):
    if name == "rot30":
        return affine_map(wr.rotation_m(w, h, 30.0), wo, ho)
    if name == "barrel":
        return barrel_map(w, h, wo, ho)
    if name == "subpixel":
        return identity_map(wo, ho, 3 * ONE // 8 + 1, -5 * ONE // 8 - 1)
    if name == "outside":
        return identity_map(wo, ho, (w + 70) * ONE, 0)                              # every position right of the image
    if name == "half-out":
        return affine_map(wr.rotation_m(w, h, 20.0, 1.0, (0.0, 0.0)), wo, ho)
    if name == "wild":
        rng = np.random.default_rng(w * 131 + wo)
        return np.stack([rng.integers(-3 * ONE, (w + 2) * ONE + 1, size=(ho, wo)), rng.integers(-3 * ONE, (h + 2) * ONE + 1, size=(ho, wo))], axis=-1).astype(np.int32)
    if name == "extremes":
        return extremes_map(w, h, wo, ho)
    raise KeyError(name)


MIXED_SHAPE, MIXED_OUT = (1, 512, 512, 1), (128, 64)


def mixed_map():
    """On a 512 x 512 x 1 input, 128 x 64 out: the identity in the left half of the output; in the right half an 8x
    reduction, px = 8 (X - 64), py = 8 Y (X counted from the half's first column, so that the positions lie INSIDE the
    image: 8 X itself would start at pixel 512, right of it, and clamp to one column).  A 64 x 32 pixel tile of the right
    half then reads 512 x 256 pixels = 128 KiB: direct; the left half is staged."""
    wo, ho = MIXED_OUT
    m = identity_map(wo, ho)
    m[:, wo // 2:, 0] -= (wo // 2) * ONE
    m[:, wo // 2:] *= 8
    return m


def make_remap(pkg, wo, ho, mode=BILINEAR, border=CONSTANT, fill=0, stage_bytes=0):
    return pkg.Remap(wo, ho, mode, border, fill, stage_bytes)
