"""Shared by test_kernel_proofs_gpu.py and test_kernel_proofs_host.py (not a test module): the pattern sets that prove the
median networks by the 0-1 principle, the check that morph_ref.py's proof images witness every window position of the
morph kernels (at the end of this file), and the numpy restatements of the definitions in include/mi_blur.h (median_ref.py,
sep_ref.py) that do not touch the product.

The 0-1 principle: a selection built only from min / max (and byte copies) commutes with every monotone map, so if it is
right on every two-valued window it is right on every window.  For radius r a window is D = 2r+1 columns of D rows; one
column is a D-bit value v whose bit b is "high" in row b.  The cyclic de Bruijn sequence B(2^D, D) holds every run of D
consecutive column values exactly once, so one image row of it shows every two-valued window exactly once.  Row y of
an image shows bit (y + phase) mod D of each column value: a window centred on an interior row sees a rotation of the
bits, which is a bijection on column values, so every interior row sees every window.
"""
import functools
import math

import numpy as np

from median_ref import ref_median  # noqa: F401  (kp.ref_median, kp.ref_sep, kp.rand_taps: the restatements the proofs use)
from sep_ref import rand_taps, ref_sep  # noqa: F401

MEDIAN_PAIRS = [(0, 255), (127, 128)]     # (low, high): any one proves the network; the second catches top-bit pack errors


def med_bh(r):
    """Output rows per lane of blur_median_fast_kernel (radius 1: 8, radius 2: 4)."""
    return 8 if r == 1 else 4


def fast_align(c):
    """Smallest pixel count whose row is a whole number of 16-byte chunks."""
    return 16 // math.gcd(c, 16)


@functools.lru_cache(maxsize=None)
def debruijn(m, n):
    """Cyclic de Bruijn sequence B(2^m, n) for prime n, by the FKM construction: the Lyndon words of length 1 and n over
    2^m letters, in lexicographic order, concatenated.  Returns uint8 (m <= 8) of length 2^(m n); the linear sequence is
    this plus its first n-1 letters."""
    assert n in (2, 3, 5, 7) and m * n <= 30
    k = 1 << m
    mask = (1 << (m * n)) - 1
    w = np.arange(1 << (m * n), dtype=np.int64)            # word w: letter j = digit j from the top, base 2^m
    rot_min = np.full_like(w, mask + 1)
    for s in range(1, n):                                   # the n-1 nontrivial rotations
        sh = m * s
        np.minimum(rot_min, ((w << sh) | (w >> (m * n - sh))) & mask, out=rot_min)
    lyndon = w < rot_min                                    # strictly below every rotation: Lyndon of length n
    const = (w % ((mask) // (k - 1))) == 0                  # aaaa...a: the Lyndon word "a" of length 1, in its place
    keep = lyndon | const
    words = w[keep]
    lens = np.where(lyndon[keep], n, 1)
    del w, rot_min, lyndon, const, keep
    starts = np.cumsum(lens) - lens
    total = int(lens.sum())
    assert total == 1 << (m * n)
    rep = np.repeat(words, lens)
    j = np.arange(total, dtype=np.int64) - np.repeat(starts, lens)
    # a constant word contributes its first letter: the top digit, like letter 0 of a length-n word
    digit = (rep >> (m * (n - 1 - j))) & (k - 1)
    return digit.astype(np.uint8)


def window_codes(seq, m, n):
    """Integer code of every run of n consecutive letters of the LINEAR sequence (seq + its first n-1 letters)."""
    lin = np.concatenate([seq, seq[:n - 1]]).astype(np.int64)
    code = np.zeros(len(seq), np.int64)
    for j in range(n):
        code = (code << m) | lin[j:j + len(seq)]
    return code


# ---------------------------------------------------------------- pattern sets (numpy form; the GPU module builds the same on the device)
CHANNEL_OFFSET = 0x2F0B5                   # stream offset of channel c: c * CHANNEL_OFFSET (odd channels also complemented)


def row_bit(y, c, d):
    """Bit of the column value that row y of channel c shows."""
    return (y + c) % d


def stream_width(r, c, shift):
    """Width of the interior-stream image: `shift` pad pixels, the 2^(D D) columns of B(2^D, D) plus 2r, rounded up to
    whole chunks."""
    d = 2 * r + 1
    w = shift + (1 << (d * d)) + 2 * r
    a = fast_align(c)
    return (w + a - 1) // a * a


def stream_mask_np(seq, r, c, shift, x0=0, w=None, h=None):
    """0/1 mask (1, H, W, C) of the interior stream: pixel x of channel c shows column value seq[(x - shift +
    c * CHANNEL_OFFSET) mod len]; row y its bit row_bit(y, c); odd channels complemented.  x0 / w crop columns."""
    d = 2 * r + 1
    h = med_bh(r) + 2 * r if h is None else h
    w = stream_width(r, c, shift) - x0 if w is None else w
    n = len(seq)
    out = np.empty((1, h, w, c), np.uint8)
    x = np.arange(x0, x0 + w, dtype=np.int64)
    for ch in range(c):
        v = seq[(x - shift + ch * CHANNEL_OFFSET) % n]
        for y in range(h):
            out[0, y, :, ch] = ((v >> row_bit(y, ch, d)) & 1) ^ (ch & 1)
    return out


def edge_width(r, c):
    """Narrowest width of whole chunks with at least 4r pixels: the first and last 2r columns are distinct."""
    a = fast_align(c)
    return max(a, (4 * r + a - 1) // a * a)


EDGE_MUL, EDGE_ADD = 0x9E3B5, 0x3A5A5      # the right edge enumerates combinations in the order i -> i * MUL + ADD (odd MUL)


def edge_combos(r):
    d = 2 * r + 1
    return 1 << (d * 2 * r)


def edge_mask_np(r, c):
    """0/1 mask (N, H, W, C) of the edge batch: image i's first 2r columns are the base-2^D digits of combination
    (i + c * CHANNEL_OFFSET) mod N, its last 2r those of a permuted combination, the columns between a fixed filler."""
    d = 2 * r + 1
    nc = edge_combos(r)
    h, w = med_bh(r) + 2 * r, edge_width(r, c)
    out = np.empty((nc, h, w, c), np.uint8)
    i = np.arange(nc, dtype=np.int64)
    for ch in range(c):
        left = (i + ch * CHANNEL_OFFSET) % nc
        right = (left * EDGE_MUL + EDGE_ADD) % nc
        cols = np.empty((nc, w), np.int64)
        for x in range(w):
            cols[:, x] = (i * 7 + x * 13 + ch) % (1 << d)
        for k in range(2 * r):
            cols[:, k] = (left >> (d * k)) & ((1 << d) - 1)
            cols[:, w - 2 * r + k] = (right >> (d * k)) & ((1 << d) - 1)
        for y in range(h):
            out[:, y, :, ch] = ((cols >> row_bit(y, ch, d)) & 1) ^ (ch & 1)
    return out


def high_count_np(mask, r):
    """Number of high values in the clamped (2r+1)^2 window of every pixel of a 0/1 mask (N, H, W, C)."""
    n, h, w, c = mask.shape
    v = np.zeros(mask.shape, np.uint8)
    for j in range(-r, r + 1):
        v += mask[:, np.clip(np.arange(h) + j, 0, h - 1)]
    p = np.concatenate([np.repeat(v[:, :, :1], r, axis=2), v, np.repeat(v[:, :, -1:], r, axis=2)], axis=2)
    cnt = np.zeros(mask.shape, np.uint8)
    for i in range(2 * r + 1):
        cnt += p[:, :, i:i + w]
    return cnt


def two_valued(mask, lo, hi):
    return np.where(mask.astype(bool), np.uint8(hi), np.uint8(lo))


def median_from_count(cnt, r, lo, hi):
    """The k-th smallest of a window of lo / hi values is hi exactly when more than k values are high."""
    k = ((2 * r + 1) ** 2 - 1) // 2
    return np.where(cnt >= k + 1, np.uint8(hi), np.uint8(lo))


# ---------------------------------------------------------------- restatements of the definitions in include/mi_blur.h
def one_hot(rb, d, b):
    """Taps of radius rb: 2^b at offset d, 0 elsewhere."""
    t = [0] * (2 * rb + 1)
    t[rb + d] = 1 << b
    return t


def shifted(img, d, axis):
    """img moved by d pixels along axis 1 (rows) or 2 (columns), clamped: out[.., x, ..] = img[.., clamp(x + d), ..]."""
    n = img.shape[axis]
    return np.take(img, np.clip(np.arange(n) + d, 0, n - 1), axis=axis)


ONE_HOT_BUCKETS = (4, 8, 16)               # blur_sep_tiled_kernel's radius buckets RB
ONE_HOT_CPR = (1, 40)                      # one chunk; more than one strip of 32 chunk columns


def chunk_cols(cpr, c):
    """cpr rounded to the nearest chunk count that whole pixels of c channels fill (a multiple of 3 for c = 3)."""
    a = fast_align(c) * c // 16                       # chunks per aligned pixel run
    return max(a, int(round(cpr / a)) * a)


def one_hot_cases():
    """(c, axis, rb, d, b, w, h): a one-hot tap 2^b at offset d of a radius-rb axis (2 = horizontal, 1 = vertical; the
    other axis [1]), on rows of one chunk column and of 40 (a tile of more than one 32-column strip)."""
    for c in range(1, 5):
        for cpr in ONE_HOT_CPR:
            w = chunk_cols(cpr, c) * 16 // c
            for axis, h in ((2, 6), (1, 40)):
                for rb in ONE_HOT_BUCKETS:
                    for d in range(-rb, rb + 1):
                        for b in (0, 8):
                            yield c, axis, rb, d, b, w, h


# ---------------------------------------------------------------- the morph proof: every window position witnessed
# A composition of minima is the minimum over a set of source positions, so blur_morph_tiled_kernel (van Herk vertically,
# doubling horizontally) is right iff the set of every output is right.  An image witnesses (position, offset d) when a
# restatement whose window differs from the true one in offset d alone gives another byte there: d inside [-r, r] is a
# window one tap short, d = -(r+1) or r+1 one tap long.
MORPH_PROOF_C = (1, 2, 3, 4)
MORPH_PROOF_RADII = tuple(range(17))
MORPH_PROOF_SQUARE = (3, 4, 16)            # (r, r): the straight vertical taps' last radius, van Herk's first, the largest


def morph_proof_cases(axis):
    """(rx, ry) of the proof on axis 2 (horizontal image) or 1 (vertical image): every radius on the proved axis with the
    other at 0, then the squares."""
    line = [(r, 0) if axis == 2 else (0, r) for r in MORPH_PROOF_RADII]
    return line + [(r, r) for r in MORPH_PROOF_SQUARE]


def window_qualifies(n, r, d):
    """Positions 0..n-1 whose source for offset d, clamped, is reached by no other offset of the clamped window [-r, r]:
    at an image edge several offsets clamp to the same pixel, and those pairs cannot be witnessed by anything."""
    x = np.arange(n)
    others = np.array([i for i in range(-r, r + 1) if i != d])
    src = np.clip(x + d, 0, n - 1)
    return ~(np.clip(x[:, None] + others[None, :], 0, n - 1) == src[:, None]).any(axis=1)


def morph_window_gaps(batch, axis, r):
    """batch (B, H, W, C) of impulse images, axis 2 (windows along x) or 1 (along y).  For every offset d of -(r+1) .. r+1
    the mutant's min and max (the window without d, or with d where it lies outside) against the true ones.  Returns the
    (image, d, position) that qualify and are NOT witnessed by that image alone: position = (x, channel) on axis 2, where
    some row must differ; = y on axis 1, where some byte of the row must differ.  Running extrema from both ends of the
    window give every mutant in two passes per tap."""
    n = batch.shape[axis]
    gaps = []
    planes = []
    for fn in (np.minimum, np.maximum):
        taps = [shifted(batch, i, axis) for i in range(-r - 1, r + 2)]           # taps[i + r + 1]
        left, right = [None] * (2 * r + 3), [None] * (2 * r + 3)                 # left[j]: offsets -r .. j - r - 1; right[j]: j - r - 1 .. r
        for j in range(1, 2 * r + 2):
            left[j] = taps[j] if j == 1 else fn(left[j - 1], taps[j])
        for j in range(2 * r + 1, 0, -1):
            right[j] = taps[j] if j == 2 * r + 1 else fn(right[j + 1], taps[j])
        true = left[2 * r + 1]
        assert np.array_equal(true, right[1])
        mutants = []
        for j in range(2 * r + 3):
            if j == 0 or j == 2 * r + 2:
                mutants.append(fn(true, taps[j]))
            elif j == 1:
                mutants.append(right[2])
            elif j == 2 * r + 1:
                mutants.append(left[2 * r])
            else:
                mutants.append(fn(left[j - 1], right[j + 1]))
        planes.append((true, mutants))
    for j, d in enumerate(range(-r - 1, r + 2)):
        differs = (planes[0][1][j] != planes[0][0]) | (planes[1][1][j] != planes[1][0])
        seen = differs.any(axis=1) if axis == 2 else differs.any(axis=(2, 3))     # (B, W, C) or (B, H)
        ok = window_qualifies(n, r, d)
        missing = ~seen & (ok[None, :, None] if axis == 2 else ok[None, :])
        gaps += [(d,) + tuple(int(v) for v in m) for m in np.argwhere(missing)[:4]]
    return gaps
