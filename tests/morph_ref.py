"""Erode / dilate / morphological gradient of include/mi_blur.h restated in numpy, independent of the product, with the
input builders tests/test_morph_host.py and tests/test_morph_gpu.py share (not a test module).

On uniformly random bytes a 33x33 minimum is 0 almost everywhere, so a window one pixel short would pass.  The builders
therefore make sparse impulses (single pixels of 0 and 255 in ONE channel on a background of 128, more than 33 apart:
erode / dilate must paint exact rectangles in that channel only), slow ramps, checkerboards and low-amplitude noise.
None of these witnesses every (byte position, offset) pair at every radius; the proof images at the end of this file do."""
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


def _ext_1d(a, r, axis, fn):
    """fn (np.minimum / np.maximum) over the 2r+1 taps along one axis, edge padding: one vectorised pass per tap."""
    if r == 0:
        return a
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    cut = lambda i: p[(slice(None),) * axis + (slice(i, i + n),)]
    out = cut(0).copy()
    for i in range(1, 2 * r + 1):
        fn(out, cut(i), out=out)
    return out


def ref_lo_hi(img, rx, ry):
    """The separable restatement (1-D windows along x, then along y); test_separable_restatement ties it to the 2-D one."""
    return (_ext_1d(_ext_1d(img, rx, 2, np.minimum), ry, 1, np.minimum),
            _ext_1d(_ext_1d(img, rx, 2, np.maximum), ry, 1, np.maximum))


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


# ---------------------------------------------------------------- proof images: every window position witnessed
# min / max compose to the min / max over a SET of source positions, so the kernel is right iff that set is right, and one
# isolated impulse shows exactly which outputs contain its position.  Impulses PROOF_PERIOD apart: more than 33 + 1, so a
# window of radius <= 16, and one a tap too long, holds at most one.  kernel_proofs.morph_window_gaps checks that the
# images witness every (position, offset) pair that anything can witness.
PROOF_PERIOD = 35
PROOF_PAIRS = [(0, 128), (255, 128), (127, 128), (128, 127)]     # (impulse, background); the last two: top bits of the 16-bit fields
PROOF_H_WIDTH = 16 * PROOF_PERIOD                                 # 560 pixels: whole chunks for 1-4 channels, 35 chunks for one
PROOF_V_SHAPE = (2 * PROOF_PERIOD, 48)                            # 70 rows (two tiles and 6 rows) x 48 pixels (whole chunks for 1-4 channels)


def _proof_batch(mask):
    return np.stack([np.where(mask, np.uint8(v), np.uint8(bg)) for v, bg in PROOF_PAIRS])


def proof_horizontal(c, period=PROOF_PERIOD, width=PROOF_H_WIDTH, drop_row=None):
    """(4, period*c, width, c): row k*c + ch has impulses at the pixels x = k (mod period) in channel ch.  gcd(period, 32)
    = 1 and width = 16 periods, so the impulses of the rows of one channel pass through every byte of the two chunks a
    thread of the horizontal pass takes, at every offset, and touch both row ends.  drop_row leaves one row without
    impulses (for showing that the sufficiency check notices)."""
    mask = np.zeros((period * c, width, c), bool)
    for k in range(period):
        for ch in range(c):
            mask[k * c + ch, k::period, ch] = k * c + ch != drop_row
    return _proof_batch(mask)


def proof_vertical(c, period=PROOF_PERIOD, shape=PROOF_V_SHAPE):
    """(4, 70, 48, c): column x has impulses at the rows y = x (mod period), in channel x % c."""
    h, w = shape
    mask = np.zeros((h, w, c), bool)
    for x in range(w):
        mask[x % period::period, x, x % c] = True
    return _proof_batch(mask)
