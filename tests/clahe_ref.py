"""CLAHE restated from the definition in include/mi_blur.h ("CLAHE"), independent of the product: np.bincount for the
tile histograms, Python integers for the clip, the redistribution and the table, a direct per-pixel blend.  Also the rules
for the two tiled kernels and the kernels' names (not a test module)."""
import numpy as np

BINS = 256
MAX_TILES = 64
ONE = 2048                  # the weights' unit per axis: 11 fraction bits
GROUP = 16                  # pixels per group: the tiled kernels' rule is W % 16 == 0 and aligned images
SPAN = 256                  # pixels per span of blur_clahe_apply_tiled_kernel: CLAHE_SPAN of csrc/filter.h
LDS_TABLE_BYTES = 32768     # the header's LDS rule: CLAHE_LDS_TABLE_BYTES of csrc/filter.h
GENERIC_BLOCKS = 16384      # workgroups of blur_clahe_tables_generic_kernel at most: CLAHE_GENERIC_BLOCKS of csrc/filter.h
TABLES_TILED, TABLES_GENERIC = "blur_clahe_tables_tiled_kernel", "blur_clahe_tables_generic_kernel"
APPLY_TILED, APPLY_GENERIC = "blur_clahe_apply_tiled_kernel", "blur_clahe_apply_generic_kernel"


def edge(S, T, t):
    """b_t: the first pixel of tile t on an axis of S pixels and T tiles."""
    return t * S // T


def mid(S, T, t):
    """m_t: the centre of tile t in half-pixels."""
    return edge(S, T, t) + edge(S, T, t + 1)


def ref_coord(S, T, x):
    """(t0, t1, frac) of pixel x, straight from the header's text."""
    p = 2 * x + 1
    if T == 1 or p <= mid(S, T, 0):
        return 0, 0, 0
    if p >= mid(S, T, T - 1):
        return T - 1, T - 1, 0
    t0 = max(t for t in range(T) if mid(S, T, t) <= p)
    return t0, t0 + 1, (p - mid(S, T, t0)) * ONE // (mid(S, T, t0 + 1) - mid(S, T, t0))


def ref_axis(S, T):
    """ref_coord for every pixel of an axis: three int64 arrays."""
    mids = [mid(S, T, t) for t in range(T)]
    t0s, t1s, fs = np.zeros(S, np.int64), np.zeros(S, np.int64), np.zeros(S, np.int64)
    for x in range(S):
        p = 2 * x + 1
        if T == 1 or p <= mids[0]:
            continue
        if p >= mids[T - 1]:
            t0s[x] = t1s[x] = T - 1
            continue
        t0 = int(np.searchsorted(mids, p, side="right")) - 1
        t0s[x], t1s[x], fs[x] = t0, t0 + 1, (p - mids[t0]) * ONE // (mids[t0 + 1] - mids[t0])
    return t0s, t1s, fs


def ref_clipped(h, A, clip_q8):
    """h' of the header's steps 1 and 2 from the 256 Python integers h that sum to A."""
    h = [int(x) for x in h]
    assert sum(h) == A and A > 0
    if clip_q8 == 0:
        return h
    clip = max(1, clip_q8 * A // 65536)
    excess = sum(max(x - clip, 0) for x in h)
    out = [min(x, clip) + excess // 256 for x in h]
    residual = excess % 256
    if residual > 0:
        step = max(256 // residual, 1)
        for v in range(BINS):
            if v % step == 0 and v // step < residual:
                out[v] += 1
    return out


def ref_table(h, A, clip_q8):
    """One tile table: step 3 on ref_clipped()."""
    hp = ref_clipped(h, A, clip_q8)
    lut, run = [], 0
    for x in hp:
        run += x
        lut.append((510 * run + A) // (2 * A))
    return lut


def tile_box(w, h, tx, ty, i, j):
    """Pixels [x0, x1) x [y0, y1) of tile (row j, column i)."""
    return edge(w, tx, i), edge(w, tx, i + 1), edge(h, ty, j), edge(h, ty, j + 1)


def ref_tables(img, tiles, clip_q8, mask=0):
    """img N x H x W x C -> (hist uint32 N x TY x TX x C x 256, tables uint8 of the same shape)."""
    n, h, w, c = img.shape
    tx, ty = tiles
    mask = mask or (1 << c) - 1
    hist = np.empty((n, ty, tx, c, BINS), np.uint32)
    tables = np.empty((n, ty, tx, c, BINS), np.uint8)
    for k in range(n):
        for j in range(ty):
            for i in range(tx):
                x0, x1, y0, y1 = tile_box(w, h, tx, ty, i, j)
                A = (x1 - x0) * (y1 - y0)
                for ch in range(c):
                    hh = np.bincount(img[k, y0:y1, x0:x1, ch].reshape(-1), minlength=BINS)
                    hist[k, j, i, ch] = hh
                    tables[k, j, i, ch] = ref_table(hh, A, clip_q8) if (mask >> ch) & 1 else np.arange(BINS)
    return hist, tables


def ref_apply(img, tables):
    """img N x H x W x C through tables N x TY x TX x C x 256: the header's blend for every pixel, in int64."""
    n, h, w, c = img.shape
    ty, tx = tables.shape[1:3]
    x0, x1, fx = ref_axis(w, tx)
    y0, y1, fy = ref_axis(h, ty)
    X0, X1, FX, Y0, Y1, FY = x0[None, :], x1[None, :], fx[None, :], y0[:, None], y1[:, None], fy[:, None]
    out = np.empty_like(img)
    for k in range(n):
        for ch in range(c):
            T = tables[k, :, :, ch, :].astype(np.int64)
            v = img[k, :, :, ch]
            acc = ((ONE - FX) * (ONE - FY) * T[Y0, X0, v] + FX * (ONE - FY) * T[Y0, X1, v] + (ONE - FX) * FY * T[Y1, X0, v] +
                   FX * FY * T[Y1, X1, v] + (1 << 21)) >> 22
            out[k, :, :, ch] = acc
    return out


def ref_clahe(img, tiles, clip_q8, mask=0):
    """(output, histograms, tables) of the whole operation."""
    hist, tables = ref_tables(img, tiles, clip_q8, mask)
    return ref_apply(img, tables), hist, tables


def work_words(n, tiles, c):
    return n * tiles[0] * tiles[1] * c * BINS


def split_work(work, n, tiles, c):
    """A work buffer's bytes -> (hist, tables)."""
    words = work_words(n, tiles, c)
    shape = (n, tiles[1], tiles[0], c, BINS)
    return work[:4 * words].view(np.uint32).reshape(shape), work[4 * words:5 * words].reshape(shape)


def tables_take_tiled(shape, offset_in=0):
    """The header's rule for blur_clahe_tables_tiled_kernel."""
    return shape[2] % GROUP == 0 and offset_in % 16 == 0


def span_cols(w, tx):
    """The most tile columns a span of SPAN pixels needs: from t0 of its first pixel to t1 of its last."""
    return max(ref_coord(w, tx, min(xa + SPAN, w) - 1)[1] - ref_coord(w, tx, xa)[0] + 1 for xa in range(0, w, SPAN))


def apply_takes_tiled(shape, tiles, offset_in=0, offset_out=0):
    """The header's rule for blur_clahe_apply_tiled_kernel, its LDS rule included."""
    n, h, w, c = shape
    return w % GROUP == 0 and offset_in % 16 == 0 and offset_out % 16 == 0 and span_cols(w, tiles[0]) * 2 * c * BINS <= LDS_TABLE_BYTES
