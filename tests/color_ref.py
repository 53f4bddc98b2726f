"""The colour transform restated in numpy from the definition in include/mi_blur.h ("Colour transform"), independent of
the product: int64 sums, an arithmetic shift, a clamp, a table.  Also the header's table of presets, the rule for
blur_color_tiled_kernel and the kernel's units (not a test module)."""
import numpy as np

MAX_CHANNELS = 4
ROW_MAX, BIAS_MAX = 1 << 18, 1 << 26
GROUP = 16                  # pixels per group: COLOR_GROUP of csrc/filter.h
RUN = 256                   # groups per workgroup: COLOR_RUN of csrc/filter.h
Q, R = 65536, 32768
TILED, GENERIC = "blur_color_tiled_kernel", "blur_color_generic_kernel"

# name -> (id, Co, shift, rows of weights, biases): the header's table, typed in from it
PRESETS = {
    "rgb2gray": (0, 1, 16, [[19595, 38470, 7471]], [R]),
    "bgr2gray": (1, 1, 16, [[7471, 38470, 19595]], [R]),
    "gray2rgb": (2, 3, 0, [[1], [1], [1]], [0, 0, 0]),
    "rgb2bgr": (3, 3, 0, [[0, 0, 1], [0, 1, 0], [1, 0, 0]], [0, 0, 0]),
    "rgba2bgra": (4, 4, 0, [[0, 0, 1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], [0, 0, 0, 0]),
    "rgba2rgb": (5, 3, 0, [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [0, 0, 0]),
    "rgb2rgba": (6, 4, 0, [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], [0, 0, 0, 255]),
    "rgb2ycbcr": (7, 3, 16, [[19595, 38470, 7471], [-11058, -21710, 32768], [32768, -27439, -5329]], [R, 128 * Q + R, 128 * Q + R]),
    "ycbcr2rgb": (8, 3, 16, [[Q, 0, 91881], [Q, -22553, -46802], [Q, 116130, 0]],
                  [R - 128 * 91881, R + 128 * (22553 + 46802), R - 128 * 116130]),
}
# the JFIF constants the integers are q() of
JFIF = {"luma": (0.299, 0.587, 0.114), "cb": (-0.168736, -0.331264, 0.5), "cr": (0.5, -0.418688, -0.081312),
        "r": 1.402, "g": (0.344136, 0.714136), "b": 1.772}


def q(x):
    return int(np.floor(x * 65536 + 0.5))


def preset(name):
    """(matrix Co x 4 int64 with zero columns beyond the preset's, bias Co, shift) of the header's table."""
    _, co, shift, rows, bias = PRESETS[name]
    m = np.zeros((co, 4), np.int64)
    for o, r in enumerate(rows):
        m[o, :len(r)] = r
    return m, np.array(bias, np.int64), shift


def ref_color(img, m, bias, shift, lut=None):
    """img N x H x W x C uint8; m Co x (>= C) integers (columns beyond C unused); bias Co; lut None or Co x 256."""
    m, bias = np.asarray(m, np.int64), np.asarray(bias, np.int64)
    c = img.shape[-1]
    acc = np.einsum("oi,...i->...o", m[:, :c], img.astype(np.int64)) + bias
    v = np.clip(acc >> shift, 0, 255)                                    # >> on int64 is arithmetic: floors
    if lut is not None:
        lut = np.asarray(lut, np.uint8)
        v = np.stack([lut[o][v[..., o]] for o in range(m.shape[0])], axis=-1)
    return v.astype(np.uint8)


def ref_preset(img, name, lut=None):
    return ref_color(img, *preset(name), lut)


def takes_tiled(shape, offset_in=0, offset_out=0):
    """The header's rule for blur_color_tiled_kernel: W * H a multiple of 16 and both pointers 16-byte aligned (the rule is
    flat: rows need not be whole chunks; dense images are then whole chunks apart)."""
    n, h, w, c = shape
    return (w * h) % GROUP == 0 and offset_in % 16 == 0 and offset_out % 16 == 0


def blocks(n, h, w):
    """Workgroups of a tiled launch: runs of RUN groups per image."""
    return n * -(-(w * h // GROUP) // RUN)


def gamma_table(gamma):
    return np.floor(255.0 * np.power(np.arange(256) / 255.0, gamma) + 0.5).astype(np.uint8)


def threshold_table(t, lo=0, hi=255):
    return np.where(np.arange(256) > t, hi, lo).astype(np.uint8)


def all_colours():
    """Every 24-bit colour once: 1 x 4096 x 4096 x 3, (r, g, b) = the three bytes of the pixel's index."""
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(1, 4096, 4096, 3)


def random_transform(rng, c, co, lut_on, shift, limit=True):
    """(m Co x 4, bias Co, shift, lut Co x 256 | None), signed weights.  With `limit` every row sums to exactly ROW_MAX
    in absolute value over its four columns and the bias is +-BIAS_MAX (most outputs then sit on the clamp); without it
    the weights are within +-1 unit of 1 << shift and the bias within +-200 units, so the outputs spread over 0..255
    and beyond both ends."""
    if limit:
        m = rng.integers(-ROW_MAX // 8, ROW_MAX // 8 + 1, size=(co, 4), dtype=np.int64)
        for o in range(co):
            k = int(rng.integers(0, c))                                   # a used column takes up the rest of the budget
            rest = ROW_MAX - (np.abs(m[o]).sum() - abs(m[o, k]))
            m[o, k] = rest if rng.integers(0, 2) else -rest
        assert (np.abs(m).sum(axis=1) == ROW_MAX).all()
        bias = rng.choice([-BIAS_MAX, BIAS_MAX], size=co)
    else:
        unit = 1 << shift
        m = rng.integers(-unit, unit + 1, size=(co, 4), dtype=np.int64)
        bias = rng.integers(-200 * unit, 200 * unit + 1, size=co)
        assert (np.abs(m).sum(axis=1) <= ROW_MAX).all() and (np.abs(bias) <= BIAS_MAX).all()
    lut = np.stack([rng.permutation(256) for _ in range(co)]).astype(np.uint8) if lut_on else None
    return m, bias.astype(np.int64), shift, lut
