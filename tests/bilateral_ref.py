"""The bilateral filter of include/mi_blur.h restated in numpy, independent of the product, with the table and input
builders tests/test_bilateral_host.py and tests/test_bilateral_gpu.py share (not a test module)."""
import numpy as np


def ref_bilateral(img, S, R):
    """The definition: img (N, H, W, C) uint8, S (2r+1, 2r+1) and R (256,) integer tables.  One vectorised pass per tap,
    uint64 sums, and the bound that makes 32-bit sums exact is asserted."""
    S = np.asarray(S, np.uint64)
    R = np.asarray(R, np.uint64)
    r = S.shape[0] // 2
    assert S.shape == (2 * r + 1, 2 * r + 1) and R.shape == (256,)
    n, h, w, c = img.shape
    p = np.pad(img, ((0, 0), (r, r), (r, r), (0, 0)), mode="edge").astype(np.int64)
    v0 = img.astype(np.int64)
    num = np.zeros(img.shape, np.uint64)
    den = np.zeros(img.shape, np.uint64)
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            if S[j, i] == 0:
                continue
            v = p[:, j:j + h, i:i + w, :]
            wgt = S[j, i] * R[np.abs(v - v0)]
            den += wgt
            num += wgt * v.astype(np.uint64)
    assert den.min() >= 1
    t = num + den // 2
    assert int(t.max()) < 2 ** 32
    return (t // den).astype(np.uint8)


def gauss_tables(sigma_space, sigma_range, radius):
    """mi_blur_bilateral_gauss in numpy's double exp."""
    if sigma_space <= 0:
        sigma_space = radius / 2.0
    i = np.arange(-radius, radius + 1, dtype=np.float64)
    d2 = i[:, None] ** 2 + i[None, :] ** 2
    S = np.floor(128.0 * np.exp(-d2 / (2.0 * sigma_space * sigma_space)) + 0.5).astype(np.int64)
    d = np.arange(256, dtype=np.float64)
    R = np.floor(255.0 * np.exp(-d * d / (2.0 * sigma_range * sigma_range)) + 0.5).astype(np.int64)
    return S, R


def random_tables(rng, radius, zeros=0.0, smax=255):
    """Random tables that pass the validation: centre and R[0] non-zero, sum S <= 65535; a share `zeros` of S is 0."""
    n = 2 * radius + 1
    hi = max(1, min(smax, 65535 // (n * n)))
    S = rng.integers(0, hi + 1, size=(n, n))
    S[rng.random((n, n)) < zeros] = 0
    S[radius, radius] = max(1, int(S[radius, radius]))
    R = rng.integers(0, 256, size=256)
    R[0] = max(1, int(R[0]))
    assert S.sum() <= 65535
    return S, R


def make_kernel(pkg, S, R):
    return pkg.Bilateral.from_tables(np.asarray(S).tolist(), np.asarray(R).tolist())


def input_kinds(rng, n, h, w, c):
    """Random bytes (every |v - v0|), low-amplitude noise, a ramp, a checkerboard."""
    yy, xx = np.mgrid[0:h, 0:w]
    return [rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8),
            rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8),
            np.broadcast_to(((xx * 7 + yy * 3) % 256).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
            np.broadcast_to((((xx + yy) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy()]


def division_images(h, w, c):
    """Two-valued images whose windows step through every split of the two values: with S all 1 and R all 255 the output
    is round_half_up((k a + (T - k) b) / T) for every count k a window can hold, so the quotients land on and beside .5
    boundaries.  Vertical stripes whose widths grow, and the same transposed, for several value pairs."""
    imgs = []
    for a, b in ((0, 255), (0, 1), (1, 2), (254, 255), (3, 250), (127, 128), (0, 2)):
        x = np.arange(w)
        stripes = (np.floor(np.sqrt(2.0 * x)) % 2).astype(bool)          # runs of 1, 2, 3, ... columns
        y = np.arange(h)
        bands = (np.floor(np.sqrt(2.0 * y)) % 2).astype(bool)
        m = stripes[None, :] ^ bands[:, None]
        img = np.where(m, a, b).astype(np.uint8)
        imgs.append(np.broadcast_to(img[:, :, None], (h, w, c)).copy())
    return np.stack(imgs)
