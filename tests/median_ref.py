"""The median blur of include/mi_blur.h restated in numpy, independent of the product, with the input builder
tests/test_median_host.py and tests/test_median_gpu.py share (not a test module)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def ref_median(img, r):
    """img (N, H, W, C) uint8: edge padding by r, every (2r+1)^2 window, the k-th smallest (k = ((2r+1)^2 - 1) / 2)."""
    d = 2 * r + 1
    p = np.pad(img, ((0, 0), (r, r), (r, r), (0, 0)), mode="edge")
    flat = sliding_window_view(p, (d, d), axis=(1, 2)).reshape(img.shape + (d * d,))
    k = (d * d - 1) // 2
    return np.partition(flat, k, axis=-1)[..., k].astype(np.uint8)


def adversarial(rng, n, h, w, c):
    """Images that stress ties and extremes: constant, salt-and-pepper, two- and few-valued, ramps, checkerboards."""
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.full((n, h, w, c), 77, np.uint8),
            np.where(rng.random((n, h, w, c)) < 0.5, 0, 255).astype(np.uint8),
            np.where(rng.random((n, h, w, c)) < 0.2, rng.choice([0, 255], (n, h, w, c)), 128).astype(np.uint8),
            rng.choice(np.array([3, 200], np.uint8), (n, h, w, c)),
            rng.choice(np.array([0, 1, 2, 254, 255], np.uint8), (n, h, w, c)),
            np.broadcast_to(((xx * 7 + yy * 3) % 256).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
            np.broadcast_to((((xx + yy) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy()]
