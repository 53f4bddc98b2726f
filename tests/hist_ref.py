"""The histogram family restated from the definitions in include/mi_blur.h ("Histogram, and tone tables made from it"),
independent of the product: np.bincount for the counts, Python integers for the tables.  Also the rule for the two tiled
kernels and their units (not a test module)."""
import numpy as np

BINS = 256
GROUP = 16                  # pixels per group: COLOR_GROUP of csrc/filter.h
RUN = 512                   # groups per run: HIST_RUN of csrc/filter.h
IMAGE_BLOCKS = 256          # workgroups the histogram kernel gives one image at most: HIST_IMAGE_BLOCKS of csrc/filter.h
EQUALIZE, STRETCH = 0, 1
CLIP_MAX = 32767
HIST_TILED, HIST_GENERIC = "blur_hist_tiled_kernel", "blur_hist_generic_kernel"
TABLES_TILED, TABLES_GENERIC = "blur_tables_tiled_kernel", "blur_tables_generic_kernel"


def ref_hist(img):
    """img N x H x W x C uint8 -> uint32 N x C x 256."""
    n, h, w, c = img.shape
    out = np.empty((n, c, BINS), np.uint32)
    for i in range(n):
        for ch in range(c):
            out[i, ch] = np.bincount(img[i, :, :, ch].reshape(-1), minlength=BINS)
    return out


def ref_table(h, mode, clip_lo=0, clip_hi=0):
    """One table from the 256 Python integers h, straight from the header's text."""
    h = [int(x) for x in h]
    N = sum(h)
    cum, run = [], 0
    for x in h:
        run += x
        cum.append(run)
    c = lambda v: cum[v] if v >= 0 else 0
    ident = list(range(BINS))
    if N == 0:
        return ident
    if mode == EQUALIZE:
        m = next(v for v in range(BINS) if h[v] > 0)
        D = N - h[m]
        if D == 0:
            return ident
        return [0 if v < m else (510 * (c(v) - h[m]) + D) // (2 * D) for v in range(BINS)]
    k_lo, k_hi = N * clip_lo // 65536, N * clip_hi // 65536
    lo = min(v for v in range(BINS) if c(v) > k_lo)
    hi = max(v for v in range(BINS) if N - c(v - 1) > k_hi)
    assert lo <= hi
    if lo == hi:
        return ident
    d = hi - lo
    return [0 if v <= lo else 255 if v >= hi else (510 * (v - lo) + d) // (2 * d) for v in range(BINS)]


def ref_tables(hist, mode, clip_lo=0, clip_hi=0, joint=0, mask=0):
    """hist C x 256 (one image) -> uint8 C x 256."""
    hist = np.asarray(hist)
    c = hist.shape[0]
    mask = mask or (1 << c) - 1
    on = [ch for ch in range(c) if (mask >> ch) & 1]
    out = np.tile(np.arange(BINS, dtype=np.uint8), (c, 1))
    if joint:
        summed = [sum(int(hist[ch, v]) for ch in on) for v in range(BINS)]
        t = ref_table(summed, mode, clip_lo, clip_hi)
        for ch in on:
            out[ch] = t
    else:
        for ch in on:
            out[ch] = ref_table(hist[ch], mode, clip_lo, clip_hi)
    return out


def ref_apply(img, tables):
    """img N x H x W x C through tables N x C x 256."""
    return np.stack([np.stack([tables[i, ch][img[i, :, :, ch]] for ch in range(img.shape[3])], axis=-1) for i in range(img.shape[0])])


def ref_tone(img, mode, clip_lo=0, clip_hi=0, joint=0, mask=0):
    """(output, histograms, tables) of the whole operation."""
    hist = ref_hist(img)
    tables = np.stack([ref_tables(hist[i], mode, clip_lo, clip_hi, joint, mask) for i in range(img.shape[0])])
    return ref_apply(img, tables), hist, tables


def takes_tiled(shape, offset_in=0, offset_out=0):
    """The header's rule for blur_hist_tiled_kernel (offset_in alone) and blur_tables_tiled_kernel: W * H a multiple of 16
    and the pointers 16-byte aligned."""
    n, h, w, c = shape
    return (w * h) % GROUP == 0 and offset_in % 16 == 0 and offset_out % 16 == 0


def blocks(n, h, w):
    """Runs of RUN groups of a tiled launch: the workgroups of blur_tables_tiled_kernel."""
    return n * -(-(w * h // GROUP) // RUN)


def hist_blocks(n, h, w):
    """Workgroups of blur_hist_tiled_kernel: one per run, but at most IMAGE_BLOCKS per image (workgroup b of a larger image
    takes runs b, b + IMAGE_BLOCKS, ...)."""
    return n * min(blocks(1, h, w), IMAGE_BLOCKS)
