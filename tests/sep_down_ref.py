"""The decimating separable filter of include/mi_blur.h restated in numpy — sep_ref.ref_sep, then the subsampling, and
nothing else (not a test module).  tests/resample_harness.py launches the filter."""
import numpy as np

from sep_ref import ref_sep

PRESETS = {0: ([1, 4, 6, 4, 1], 2), 1: ([0, 1, 1], 2), 2: ([0, 0, 0, 1, 1, 1, 1], 4)}     # MI_BLUR_DOWN_*: taps of both axes, stride
PHASES = [(sx, sy, ox, oy) for sx in range(1, 5) for sy in range(1, 5) for ox in range(sx) for oy in range(sy)]


def ref_sep_down(img, wx, wy, sx=2, sy=2, ox=0, oy=0, rows=None, first_row=0):
    """img (N, H, W, C) uint8: the separable filter on the whole image, of which row oy + Y*sy and column ox + X*sx are kept.
    rows = (Y0, Y1): output rows Y0 .. Y1 - 1 only, from a slab: img then holds the image's rows from first_row on, and must
    hold the input rows of those outputs with len(wy) // 2 rows above and below as far as the image has them (where the
    slab ends at the image's edge, the padding is the image's own clamp)."""
    full = ref_sep(img, wx, wy)
    if rows is not None:
        first = oy + rows[0] * sy - first_row
        assert first >= 0 and first + (rows[1] - rows[0] - 1) * sy < img.shape[1]
        return np.ascontiguousarray(full[:, first:first + (rows[1] - rows[0] - 1) * sy + 1:sy, ox::sx, :])
    return np.ascontiguousarray(full[:, oy::sy, ox::sx, :])


def down_shape(shape, sx, sy, ox, oy):
    n, h, w, c = shape
    return n, (h - oy + sy - 1) // sy, (w - ox + sx - 1) // sx, c
