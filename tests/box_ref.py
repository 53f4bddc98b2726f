"""The integral images and the box filters restated from the definitions in include/mi_blur.h ("Integral images, and box
filters"), independent of the product and of the five-term form: np.cumsum for the tables, edge padding and sliding sums
for the windows, Python / numpy integers for the three rules.  Also the kernels' constants and routing rules for the
shape lists (not a test module)."""
import numpy as np

MEAN, STDDEV, THRESHOLD = 0, 1, 2
MAX_RADIUS = 127
BAND = 16                   # rows per band: INTEGRAL_BAND of csrc/filter.h
PIXELS = 16                 # pixels per thread: INTEGRAL_PIXELS
MAX_W = 8192                # the widest image of the tiled integral: INTEGRAL_MAX_W
WAVE_SPAN = 64 * PIXELS     # pixels one wave spans
INTEGRAL_TILED, INTEGRAL_GENERIC = "blur_integral_tiled_kernel", "blur_integral_generic_kernel"
BOX_TILED, BOX_GENERIC = "blur_box_tiled_kernel", "blur_box_generic_kernel"
M32 = 1 << 32


def ref_integral(img, square=False):
    """img N x H x W x C uint8 -> uint32 N x H x W x C: the inclusive sums modulo 2^32."""
    v = img.astype(np.uint64)
    if square:
        v = v * v
    return (np.cumsum(np.cumsum(v, axis=1, dtype=np.uint64), axis=2, dtype=np.uint64) % M32).astype(np.uint32)


def ref_integral_rows(img, starts, band, square=False, chunk=64):
    """Rows r .. r + band - 1 of the table of ONE image (H x W x C uint8) for every r of `starts`, without the table: the
    column sums of all rows above r as int64, taken `chunk` rows at a time and carried from one start to the next, then a
    cumulative sum down the band and along the row, modulo 2^32.  {r: uint32 band x W x C}.  The numpy twin of
    torch_integral_rows()."""
    above, done, out = np.zeros(img.shape[1:], np.int64), 0, {}
    for r in sorted(starts):
        while done < r:
            v = img[done:min(done + chunk, r)].astype(np.int64)
            above += (v * v if square else v).sum(axis=0)
            done += v.shape[0]
        v = img[r:r + band].astype(np.int64)
        rows = above[None] + np.cumsum(v * v if square else v, axis=0)
        out[r] = (np.cumsum(rows, axis=1) % M32).astype(np.uint32)
    return out


def torch_integral_rows(torch, d_img, starts, band, square=False, chunk=2048):
    """ref_integral_rows() on a device tensor (H x W x C uint8), in torch and nothing of the product's: {r: int64 band x W x C
    on the device, values modulo 2^32}.  A chunk of 2048 rows of 32768 bytes is 512 MiB as int64."""
    above, done, out = torch.zeros(d_img.shape[1:], dtype=torch.int64, device=d_img.device), 0, {}
    for r in sorted(starts):
        while done < r:
            v = d_img[done:min(done + chunk, r)].to(torch.int64)
            above += (v * v if square else v).sum(dim=0)
            done += v.shape[0]
            del v
        v = d_img[r:r + band].to(torch.int64)
        rows = above.unsqueeze(0) + torch.cumsum(v * v if square else v, dim=0)
        out[r] = torch.cumsum(rows, dim=1) % M32
    return out


def window_sums(img, rx, ry, square=False):
    """Sum (or SumSq) of every clamped window, int64 N x H x W x C: the image padded with its edge, then differences of an
    int64 cumulative sum of the padded image (exact: at most 65025 * 65025 per window)."""
    v = img.astype(np.int64)
    if square:
        v = v * v
    p = np.pad(v, ((0, 0), (ry, ry), (rx, rx), (0, 0)), mode="edge")
    c = np.zeros((p.shape[0], p.shape[1] + 1, p.shape[2] + 1, p.shape[3]), np.int64)
    c[:, 1:, 1:] = np.cumsum(np.cumsum(p, axis=1), axis=2)
    h, w = img.shape[1], img.shape[2]
    ky, kx = 2 * ry + 1, 2 * rx + 1
    return c[:, ky:ky + h, kx:kx + w] - c[:, :h, kx:kx + w] - c[:, ky:ky + h, :w] + c[:, :h, :w]


def ref_stddev(A, S, Q):
    """The largest s in 0..128 with s == 0 or (2 s - 1)^2 A^2 <= 4 D, D = A Q - S^2 (int64 arrays; everything below 2^63)."""
    D = A * Q - S * S
    assert (D >= 0).all()
    out = np.zeros(D.shape, np.int64)
    for s in range(1, 129):
        out[(2 * s - 1) ** 2 * A * A <= 4 * D] = s
    return out


def ref_value(op, A, S, Q=0, a=0, offset=0, invert=0):
    """The three rules on integers or int64 arrays."""
    if op == MEAN:
        return (2 * S + A) // (2 * A)
    if op == STDDEV:
        return ref_stddev(A, np.asarray(S, np.int64), np.asarray(Q, np.int64))
    on = A * (a + offset) > S
    return np.where(on != bool(invert), 255, 0)


def ref_box(img, op, rx, ry, offset=0, invert=0):
    """img N x H x W x C uint8 -> uint8 of the same shape."""
    A = (2 * rx + 1) * (2 * ry + 1)
    S = window_sums(img, rx, ry)
    Q = window_sums(img, rx, ry, True) if op == STDDEV else 0
    return np.asarray(ref_value(op, A, S, Q, img.astype(np.int64), offset, invert)).astype(np.uint8)


def integral_takes_tiled(shape, offset_in=0):
    """The header's rule for blur_integral_tiled_kernel: W a multiple of 16, at most MAX_W, an aligned input."""
    n, h, w, c = shape
    return w % PIXELS == 0 and w <= MAX_W and offset_in % 16 == 0


def box_takes_tiled(shape, offset_in=0, offset_out=0):
    """... and for blur_box_tiled_kernel: rows of whole 16-byte chunks, aligned output and input."""
    n, h, w, c = shape
    return (w * c) % 16 == 0 and offset_in % 16 == 0 and offset_out % 16 == 0


def work_bytes(shape, tables, band=BAND):
    n, h, w, c = shape
    return n * -(-h // band) * tables * w * c * 4
