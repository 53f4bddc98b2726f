"""Erode / dilate / morphological gradient of include/mi_blur.h restated in numpy, independent of the product, with the
input builders tests/test_morph_host.py and tests/test_morph_gpu.py share (not a test module).

On uniformly random bytes a 33x33 minimum is 0 almost everywhere, so a window one pixel short would pass.  The builders
therefore make sparse impulses (single pixels of 0 and 255 in ONE channel on a background of 128, more than 33 apart:
erode / dilate must paint exact rectangles in that channel only), slow ramps, checkerboards and low-amplitude noise."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

ERODE, DILATE, GRADIENT = 0, 1, 2
OPS = (ERODE, DILATE, GRADIENT)
TILE_ROWS, TILE_CHUNKS = 32, 32                                   # blur_morph_tiled_kernel's tile: output rows x 16-byte chunk columns


def _finish(lo, hi, op):
    return lo if op == ERODE else hi if op == DILATE else (hi.astype(np.int16) - lo.astype(np.int16)).astype(np.uint8)


def ref_morph_2d(img, op, rx, ry):
    """The definition: img (N, H, W, C) uint8, edge padding by (ry, rx), min / max over every full 2-D window."""
    p = np.pad(img, ((0, 0), (ry, ry), (rx, rx), (0, 0)), mode="edge")
    win = sliding_window_view(p, (2 * ry + 1, 2 * rx + 1), axis=(1, 2))
    return _finish(win.min(axis=(-2, -1)), win.max(axis=(-2, -1)), op)


def ref_lo_hi(img, rx, ry):
    """The separable restatement (1-D windows along x, then along y); test_separable_restatement ties it to the 2-D one."""
    p = np.pad(img, ((0, 0), (0, 0), (rx, rx), (0, 0)), mode="edge")
    wx = sliding_window_view(p, 2 * rx + 1, axis=2)
    lo, hi = wx.min(axis=-1), wx.max(axis=-1)
    lo = sliding_window_view(np.pad(lo, ((0, 0), (ry, ry), (0, 0), (0, 0)), mode="edge"), 2 * ry + 1, axis=1).min(axis=-1)
    hi = sliding_window_view(np.pad(hi, ((0, 0), (ry, ry), (0, 0), (0, 0)), mode="edge"), 2 * ry + 1, axis=1).max(axis=-1)
    return lo, hi


def ref_morph(img, op, rx, ry):
    return _finish(*ref_lo_hi(img, rx, ry), op)


def impulse_batch(h, w, c, candidates):
    """Images of 128 with single pixels of 0 / 255 (alternating) in one channel each at the candidate (y, x) positions;
    positions closer than 34 in both axes go to different images, so every image's impulses are more than 33 apart."""
    images = []                                                  # [(array, [(y, x), ...])]
    for k, (y, x) in enumerate(dict.fromkeys((min(max(y, 0), h - 1), min(max(x, 0), w - 1)) for y, x in candidates)):
        for img, taken in images:
            if all(max(abs(y - yy), abs(x - xx)) > 33 for yy, xx in taken):
                break
        else:
            img, taken = np.full((h, w, c), 128, np.uint8), []
            images.append((img, taken))
        img[y, x, k % c] = 0 if k % 2 else 255
        taken.append((y, x))
    return np.stack([img for img, _ in images])


def corner_impulses(h, w, c):
    cand = [(y, x) for y in (0, h // 2, h - 1) for x in (0, w // 2, w - 1)] + [(h // 3, w // 4), (1, 1), (h - 2, w - 2)]
    return impulse_batch(h, w, c, cand)


def seam_impulses(h, w, c, rx, ry):
    """Impulses on the image's edges, on both sides of every seam between tiles (rows and chunk columns) and in the first and
    last 16-byte chunk of the 64-slot groups one wave stages (slot = staged row * staged chunk columns + chunk)."""
    cpr = w * c // 16
    nstrips = -(-cpr // TILE_CHUNKS) if cpr else 1
    ncols = -(-cpr // nstrips) if cpr else 1
    hc = max(1, -(-rx * c // 16))
    rows = sorted({0, h - 1, h // 2} | {y for s in range(TILE_ROWS, h, TILE_ROWS) for y in (s - 1, s)})
    cols = sorted({0, w - 1, w // 2} | {x for s in range(ncols, cpr, ncols) for x in ((s * 16 - 1) // c, -(-s * 16 // c))})
    cand = [(y, x) for y in rows for x in cols]
    ncw = min(ncols, cpr) + 2 * hc
    for s in (63, 64, 127, 128, 64 * ((TILE_ROWS + 2 * ry) * ncw // 64) - 1, 64 * ((TILE_ROWS + 2 * ry) * ncw // 64)):
        row, cc = divmod(s, ncw)
        for b in (0, 15):
            cand.append((row - ry, ((cc - hc) * 16 + b) // c))   # first tile: staged row 0 is image row -ry (clamped away)
    return impulse_batch(h, w, c, cand)


def structured(rng, n, h, w, c, sparse_and_constant=False):
    """Ramps, checkerboards (the median tests' adversarial() list) and noise of low amplitude: the extremum depends on the
    extent.  sparse_and_constant adds sparse salt and pepper on 128 and a constant image (two more draws from rng)."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = [np.broadcast_to(((xx * 7 + yy * 3) % 256).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
           np.broadcast_to((((xx + yy) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
           rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8)]
    if sparse_and_constant:
        out += [np.where(rng.random((n, h, w, c)) < 0.02, rng.choice([0, 255], (n, h, w, c)), 128).astype(np.uint8),
                np.full((n, h, w, c), 77, np.uint8)]
    return out


def mixed(rng, n, h, w, c):
    """One batch with everything in it: low-amplitude noise, a ramp, a checkerboard, sparse salt and pepper on top."""
    yy, xx = np.mgrid[0:h, 0:w]
    img = rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8)
    img[0] = ((xx * 7 + yy * 3) % 256).astype(np.uint8)[:, :, None]
    if n > 1:
        img[1, : h // 2] = (((xx + yy) % 2) * 255).astype(np.uint8)[: h // 2, :, None]
    sp = rng.random((n, h, w, c)) < 0.002
    img[sp] = rng.choice(np.array([0, 255], np.uint8), int(sp.sum()))
    return img
