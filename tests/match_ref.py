"""Template matching and the peak search restated from include/mi_blur.h ("Template matching and peak search") in numpy
and Python integers: no product code, and no float anywhere in a score."""
import math

import numpy as np

SQDIFF, CCORR, SAD, NCC, ZNCC = range(5)
METHODS = {"sqdiff": SQDIFF, "ccorr": CCORR, "sad": SAD, "ncc": NCC, "zncc": ZNCC}
MAX_SIDE, MAX_AREA, ONE = 255, 65536, 16384
TILE = (64, 16)                                  # blur_match_tiled_kernel: MATCH_TX, MATCH_TY (csrc/filter.h)


def valid(method, tw, th, W, H, C):
    return method in range(5) and 1 <= tw <= min(W, MAX_SIDE) and 1 <= th <= min(H, MAX_SIDE) and tw * th * C <= MAX_AREA


def score(method, A, sum_at, sum_a, sum_aa, sum_t, sum_tt):
    """sign(N) k: k the largest integer in 0..16384 that is 0 or has (2k - 1)^2 D <= 2^30 N^2."""
    if method == NCC:
        N, D = sum_at, sum_aa * sum_tt
    else:
        N = A * sum_at - sum_a * sum_t
        D = (A * sum_aa - sum_a * sum_a) * (A * sum_tt - sum_t * sum_t)
    if D == 0 or N == 0:
        return 0
    rhs = (N * N) << 30
    # (2k - 1)^2 D <= rhs  <=>  2k - 1 <= isqrt(rhs // D)
    k = min((math.isqrt(rhs // D) + 1) // 2, ONE)
    assert k == 0 or (2 * k - 1) ** 2 * D <= rhs
    assert k == ONE or (2 * k + 1) ** 2 * D > rhs
    return k if N > 0 else -k


def value(method, A, sum_at, sum_a, sum_aa, sum_t, sum_tt):
    """mi_blur_match_value: None where it answers INT32_MIN."""
    if method not in (NCC, ZNCC) or not 1 <= A <= MAX_AREA:
        return None
    for s, ss in ((sum_a, sum_aa), (sum_t, sum_tt)):
        if s > 255 * A or ss > 65025 * A or s * s > A * ss:
            return None
    if sum_at * sum_at > sum_aa * sum_tt:
        return None
    return score(method, A, sum_at, sum_a, sum_aa, sum_t, sum_tt)


def match(images, templates, method):
    """images (N, H, W, C) uint8; templates (th, tw, C), shared, or (N, th, tw, C).  (N, Ho, Wo) uint32 or int32."""
    n, H, W, C = images.shape
    shared = templates.ndim == 3
    th, tw = templates.shape[-3], templates.shape[-2]
    assert valid(method, tw, th, W, H, C)
    Ho, Wo = H - th + 1, W - tw + 1
    out = np.empty((n, Ho, Wo), np.int32 if method >= NCC else np.uint32)
    A = tw * th * C
    for i in range(n):
        t = (templates if shared else templates[i]).astype(np.int64)
        st, stt = int(t.sum()), int((t * t).sum())
        win = np.lib.stride_tricks.sliding_window_view(images[i], (th, tw), axis=(0, 1))      # (Ho, Wo, C, th, tw)
        a = win.transpose(0, 1, 3, 4, 2).astype(np.int64)                                     # (Ho, Wo, th, tw, C)
        if method == SQDIFF:
            out[i] = ((a - t) ** 2).sum(axis=(2, 3, 4))
        elif method == SAD:
            out[i] = np.abs(a - t).sum(axis=(2, 3, 4))
        else:
            at = (a * t).sum(axis=(2, 3, 4))
            if method == CCORR:
                out[i] = at
            else:
                sa, saa = a.sum(axis=(2, 3, 4)), (a * a).sum(axis=(2, 3, 4))
                for y in range(Ho):
                    for x in range(Wo):
                        out[i, y, x] = score(method, A, int(at[y, x]), int(sa[y, x]), int(saa[y, x]), st, stt)
    return out


def peak(table):
    """(N, Ho, Wo) uint32 or int32 -> int64 (N, 6): min, min_x, min_y, max, max_x, max_y; the first entry wins a tie."""
    n, Ho, Wo = table.shape
    out = np.empty((n, 6), np.int64)
    for i in range(n):
        flat = table[i].reshape(-1).astype(np.int64)
        lo, hi = int(np.argmin(flat)), int(np.argmax(flat))                                   # numpy: the first occurrence
        out[i] = (flat[lo], lo % Wo, lo // Wo, flat[hi], hi % Wo, hi // Wo)
    return out
