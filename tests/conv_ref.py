"""The signed 2-D convolution of include/mi_blur.h restated in numpy, independent of the product, with the kernel and input
builders tests/test_conv_host.py and tests/test_conv_gpu.py share (not a test module)."""
import numpy as np

MODES = ("sat", "abs", "mag")


def ref_conv(img, K, shift=0, bias=0, mode="sat", K2=None):
    """The definition: img (N, H, W, C) uint8, K (2 ry + 1, 2 rx + 1) integer taps (K2 likewise, mode "mag" only).
    Correlation, clamp-to-edge.  One vectorised pass per non-zero tap, int64 sums, and the bounds that make 24-bit
    multiplies and 32-bit sums exact are asserted."""
    K = np.asarray(K, np.int64)
    assert K.ndim == 2 and K.shape[0] % 2 == 1 and K.shape[1] % 2 == 1 and max(K.shape) <= 15
    assert mode in MODES and (K2 is not None) == (mode == "mag")
    assert 0 <= shift <= 16 and abs(bias) <= 2 ** 24
    ry, rx = K.shape[0] // 2, K.shape[1] // 2
    n, h, w, c = img.shape
    p = np.pad(img, ((0, 0), (ry, ry), (rx, rx), (0, 0)), mode="edge").astype(np.int64)

    def accumulate(T):
        T = np.asarray(T, np.int64)
        assert T.shape == K.shape and np.abs(T).sum() <= 65535 and np.abs(T).max(initial=0) <= 32768
        acc = np.zeros(img.shape, np.int64)
        for j in range(T.shape[0]):
            for i in range(T.shape[1]):
                if T[j, i]:
                    acc += T[j, i] * p[:, j:j + h, i:i + w, :]
        assert np.abs(acc).max(initial=0) < 2 ** 24
        return acc

    a = accumulate(K)
    if mode != "sat":
        a = np.abs(a)
    if mode == "mag":
        a = a + np.abs(accumulate(K2))
    a = a + int(bias)
    assert np.abs(a).max(initial=0) < 2 ** 27
    return np.clip(a >> int(shift), 0, 255).astype(np.uint8)            # >> on int64 is the floor


def random_table(rng, rx, ry, zeros=0.0):
    """Signed taps over (2 ry + 1) x (2 rx + 1) with sum |K| <= 65535: small ones, 8-bit ones or as large as the bound allows."""
    n = (2 * rx + 1) * (2 * ry + 1)
    hi = (4, 127, 65535 // n)[int(rng.integers(0, 3))]
    hi = max(1, min(hi, 65535 // n, 32767))
    T = rng.integers(-hi, hi + 1, size=(2 * ry + 1, 2 * rx + 1))
    T[rng.random(T.shape) < zeros] = 0
    assert np.abs(T).sum() <= 65535
    return T


def random_kernel(rng, rx, ry, zeros=0.0, mode="sat"):
    """A kernel that passes the validation, as the keyword arguments of ref_conv / make_kernel."""
    shift = int(rng.integers(0, 17)) if rng.random() < 0.3 else int(rng.integers(0, 9))
    bias = (0, (1 << shift) >> 1, 128 << shift, int(rng.integers(-2 ** 24, 2 ** 24 + 1)),
            int(rng.integers(-4096, 4097)))[int(rng.integers(0, 5))]
    bias = max(-2 ** 24, min(2 ** 24, bias))
    return dict(K=random_table(rng, rx, ry, zeros), shift=shift, bias=bias, mode=mode,
                K2=random_table(rng, rx, ry, zeros) if mode == "mag" else None)


def make_kernel(pkg, K, shift=0, bias=0, mode="sat", K2=None):
    return pkg.Conv.from_taps(np.asarray(K).tolist(), shift, bias, mode, None if K2 is None else np.asarray(K2).tolist())


def input_kinds(rng, n, h, w, c):
    """Random bytes, low-amplitude noise, a ramp, a checkerboard."""
    yy, xx = np.mgrid[0:h, 0:w]
    return [rng.integers(0, 256, size=(n, h, w, c), dtype=np.uint8),
            rng.integers(100, 141, size=(n, h, w, c), dtype=np.uint8),
            np.broadcast_to(((xx * 7 + yy * 3) % 256).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy(),
            np.broadcast_to((((xx + yy) % 2) * 255).astype(np.uint8)[None, :, :, None], (n, h, w, c)).copy()]


def saturation_cases(h, w, c):
    """(image, kernel) pairs at the ends of the accumulator and on both sides of 0 and 255 after the shift:
    acc = +-65535 * 255 with bias +-2^24, and one-tap kernels on a ramp whose outputs cross 0 and 255."""
    full = np.full((15, 15), 291, np.int64)
    full.reshape(-1)[:65535 - 291 * 225] += 1
    assert full.sum() == 65535
    white = np.full((1, h, w, c), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.broadcast_to(((xx + yy * w) % 256).astype(np.uint8)[None, :, :, None], (1, h, w, c)).copy()
    one = lambda v: np.array([[v]], np.int64)
    cases = []
    for sign in (1, -1):
        for mode in MODES:
            K2 = -sign * full if mode == "mag" else None
            for shift, bias in ((16, 2 ** 24), (16, -2 ** 24), (16, 0), (0, 0), (16, (1 << 15)), (15, -2 ** 24 + 65535 * 255)):
                cases.append((white, dict(K=sign * full, shift=shift, bias=bias, mode=mode, K2=K2)))   # mag: 2 * 16711425 + 2^24 < 2^27
                cases.append((ramp, dict(K=sign * full, shift=shift, bias=bias, mode=mode, K2=K2)))
    for mode in ("sat", "abs"):
        for k, shift, bias in ((1, 0, -1), (1, 0, 1), (1, 0, -128), (2, 0, -255), (2, 1, 0), (2, 1, 1), (3, 1, -129), (-1, 0, 255), (-1, 0, 256),
                               (-1, 3, 43), (-1, 3, 0), (-3, 4, 2047), (-1, 16, -1), (257, 8, 0), (257, 8, 128), (-32768, 15, 2 ** 24)):
            cases.append((ramp, dict(K=one(k), shift=shift, bias=bias, mode=mode, K2=None)))
    return cases
