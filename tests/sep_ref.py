"""The separable kernels of include/mi_blur.h restated in numpy, independent of the product, with the tap builders
tests/test_sep_host.py, tests/test_sep_gpu.py, tests/test_narrow_rows_gpu.py and tests/kernel_proofs.py share (not a test
module)."""
import math

import numpy as np


def ref_taps(sigma, radius=0, bits=8):
    """mi_blur_gauss_taps as the header defines it; None where it must return MI_BLUR_ERR_INVALID."""
    if not sigma > 0 or not 0 <= radius <= 16 or not 0 <= bits <= 8:
        return None
    r = radius or min(16, max(1, math.ceil(3 * sigma)))
    w = np.array([math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)])
    t = np.floor(w * (1 << bits) / w.sum() + 0.5).astype(np.int64)
    t[r] += (1 << bits) - t.sum()
    if t[r] <= 0:
        return None
    while r > 0 and t[0] == 0 and t[-1] == 0:
        t, r = t[1:-1], r - 1
    return t.tolist()


def ref_sep(img, wx, wy):
    """img (N, H, W, C) uint8: edge padding, exact int64 sums, one shift by log2(sum wx) + log2(sum wy)."""
    rx, ry = len(wx) // 2, len(wy) // 2
    shift = int(sum(wx)).bit_length() - 1 + int(sum(wy)).bit_length() - 1
    n, h, w, c = img.shape
    p = np.pad(img.astype(np.int64), ((0, 0), (ry, ry), (rx, rx), (0, 0)), mode="edge")
    hs = sum(int(wx[i]) * p[:, :, i:i + w, :] for i in range(2 * rx + 1))
    vs = sum(int(wy[j]) * hs[:, j:j + h, :, :] for j in range(2 * ry + 1))
    return (vs >> shift).astype(np.uint8)


def rand_taps(rng, r, bits=8):
    """2r+1 non-negative taps summing to 2^bits (asymmetric).  Radius 0 draws nothing from rng."""
    if r == 0:
        return [1 << bits]
    cuts = np.sort(rng.integers(0, (1 << bits) + 1, size=2 * r))
    return np.diff(np.concatenate([[0], cuts, [1 << bits]])).tolist()
