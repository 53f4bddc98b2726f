"""The two-image arithmetic restated from the table in include/mi_blur.h ("Two-image arithmetic"), independent of the
product: numpy int64 and floor division, none of the product's shifts-for-divisions.  Also the routing rule of the three
kernels, their units, and what the two test modules share to make operands (not a test module)."""
import numpy as np

LINEAR, ABSDIFF, MIN, MAX, MUL, LERP = range(6)
# preset -> (id, op, wa, wb, bias, shift), the issue's table
PRESETS = {"add": (0, LINEAR, 1, 1, 0, 0), "sub": (1, LINEAR, 1, -1, 0, 0), "avg": (2, LINEAR, 1, 1, 1, 1), "diff128": (3, LINEAR, 1, -1, 128, 0),
           "absdiff": (4, ABSDIFF, 1, 0, 0, 0), "min": (5, MIN, 0, 0, 0, 0), "max": (6, MAX, 0, 0, 0, 0), "mul255": (7, MUL, 257, 0, 32896, 16),
           "mulq7": (8, MUL, 1, 0, 64, 7), "lerp": (9, LERP, 0, 0, 0, 0)}
MAX_W, MAX_W_MUL, MAX_BIAS, MAX_SHIFT = 1 << 16, 1 << 10, 1 << 26, 16
CHUNK = 16                  # bytes per chunk: ARITH_CHUNK of csrc/filter.h
RUN = 256                   # chunks per workgroup of the flat kernel: ARITH_RUN
PLANE_RUN = 256             # groups per workgroup of the plane kernel: ARITH_PLANE_RUN
GROUP = 16                  # pixels per group: COLOR_GROUP
FLAT, PLANE, GENERIC = "blur_arith_flat_kernel", "blur_arith_plane_kernel", "blur_arith_generic_kernel"


def ref_value(spec, a, b, m=0):
    """spec = (op, wa, wb, bias, shift); a, b, m integers or integer arrays -> int64."""
    op, wa, wb, bias, shift = spec
    a, b, m = (np.asarray(v, dtype=np.int64) for v in (a, b, m))
    if op == LINEAR:
        return np.clip((wa * a + wb * b + bias) // (1 << shift), 0, 255)
    if op == ABSDIFF:
        return np.clip((wa * np.abs(a - b) + bias) // (1 << shift), 0, 255)
    if op == MIN:
        return np.minimum(a, b)
    if op == MAX:
        return np.maximum(a, b)
    if op == MUL:
        return np.clip((wa * a * b + bias) // (1 << shift), 0, 255)
    assert op == LERP
    return (2 * (a * m + b * (255 - m)) + 255) // 510


def ref_arith(spec, a, b, m=None):
    """a: (N, H, W, C) uint8; b and m: (N or 1, H, W, C or 1), which numpy broadcasts as the definition indexes them."""
    return np.broadcast_to(ref_value(spec, a, b, 0 if m is None else m), a.shape).astype(np.uint8)


def struct_of(pkg, spec, b=None, m=None, shape=None):
    """pkg.Arith of spec, with the plane / shared flags of the operand arrays b and m against a's shape."""
    k = pkg.Arith(*spec)
    if b is not None:
        k.b_plane, k.b_shared = int(b.shape[3] != shape[3]), int(b.shape[0] != shape[0])
    if m is not None:
        k.m_plane, k.m_shared = int(m.shape[3] != shape[3]), int(m.shape[0] != shape[0])
    return k


def operand(rng, shape, plane, shared):
    n, h, w, c = shape
    return rng.integers(0, 256, size=(1 if shared else n, h, w, 1 if plane else c), dtype=np.uint8)


def random_spec(rng, op):
    """A valid struct's (op, wa, wb, bias, shift), half of the time at a limit of each field."""
    if op in (MIN, MAX, LERP):
        return (op, 0, 0, 0, 0)

    def pick(lim):
        return int(rng.choice([-lim, lim])) if rng.integers(0, 2) else int(rng.integers(-lim, lim + 1))
    lim_w = MAX_W_MUL if op == MUL else MAX_W
    shift = int(rng.choice([0, MAX_SHIFT])) if rng.integers(0, 3) == 0 else int(rng.integers(0, MAX_SHIFT + 1))
    return (op, pick(lim_w), pick(MAX_W) if op == LINEAR else 0, pick(MAX_BIAS), shift)


def lively_spec(rng, op):
    """A valid struct whose output is not mostly saturated: small weights, a shift that brings the sum back to bytes."""
    if op in (MIN, MAX, LERP):
        return (op, 0, 0, 0, 0)
    shift = int(rng.integers(4, 13))
    one = 1 << shift
    if op == LINEAR:
        wa = int(rng.integers(-one, one + 1))
        return (op, wa, int(rng.integers(-one, one + 1)), int(rng.integers(0, 128)) * one, shift)
    if op == ABSDIFF:
        return (op, int(rng.integers(1, 2 * one + 1)), 0, int(rng.integers(-one, one + 1)), shift)
    return (op, int(rng.integers(1, min(MAX_W_MUL, one) + 1)), 0, int(rng.integers(0, one)), min(shift + 7, MAX_SHIFT))


def plane_flags(k, c):
    """(b_plane, m_plane) as the launch sees them: a plane of a one-channel image is a full operand."""
    return (0, 0) if c == 1 else (k.b_plane, k.m_plane)


def takes_flat(shape, k, offsets=(0, 0, 0, 0)):
    """The header's rule for blur_arith_flat_kernel: no plane operand, W * H * C a multiple of 16, every pointer aligned."""
    n, h, w, c = shape
    return not any(plane_flags(k, c)) and (w * h * c) % CHUNK == 0 and all(o % 16 == 0 for o in offsets)


def takes_plane(shape, k, offsets=(0, 0, 0, 0)):
    """... and for blur_arith_plane_kernel: a plane operand on 2..4 channels, W * H a multiple of 16, every pointer aligned."""
    n, h, w, c = shape
    return any(plane_flags(k, c)) and (w * h) % GROUP == 0 and all(o % 16 == 0 for o in offsets)


def blocks(shape, k):
    """Workgroups of a tiled launch: runs of RUN chunks (flat) or of PLANE_RUN groups of 16 pixels (plane), per image."""
    n, h, w, c = shape
    if any(plane_flags(k, c)):
        return n * -(-(w * h // GROUP) // PLANE_RUN)
    return n * -(-(w * h * c // CHUNK) // RUN)
