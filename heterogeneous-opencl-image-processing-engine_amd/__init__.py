"""MI355X-native image-stream blur engine — build + ctypes binding of the C ABI.

The product is ``libmi_blur.so`` (HIP kernels for gfx950 behind ``include/mi_blur.h``)
and the two C++ hosts under ``apps/``.  This module is only the harness-side binding
used by tests/ and bench.py: it adds no behaviour of its own and has NO CPU fallback —
if the shared library is missing or a GPU entry point is called without a GPU, it raises.

The directory name contains hyphens, so import it with ``__graft_entry__.load_package()``
(which registers it as module ``hoipe_amd``).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
APPS = os.path.join(PKG_DIR, "apps")
LIB_PATH = os.path.join(PKG_DIR, "libmi_blur.so")
HEADER = os.path.join(ROOT, "include", "mi_blur.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# Kernel arguments in host memory: the launch-rate-bound batch stream issues ~2x faster (see the constructor in
# csrc/mi_blur_api.cpp).  Must be in the environment before the HIP runtime initialises; the user's value wins.
os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "0")
ARCH = "gfx950"

DEVICE_CPU = -1
VARIANT_AUTO, VARIANT_GENERIC, VARIANT_TILED, VARIANT_STREAM, VARIANT_DIRECT = 0, 1, 2, 3, 4
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_NOMEM, ERR_STATE, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
UNIQUE_ID_BYTES = 128
SEP_MAX_RADIUS = 16
MEDIAN_MAX_RADIUS = 7
MORPH_MAX_RADIUS = 16
MORPH_ERODE, MORPH_DILATE, MORPH_GRADIENT = 0, 1, 2
BILATERAL_MAX_RADIUS = 8
CONV_MAX_RADIUS = 7
CONV_SAT, CONV_ABS, CONV_MAG = 0, 1, 2
CONV_MODES = {"sat": CONV_SAT, "abs": CONV_ABS, "mag": CONV_MAG}
CONV_PRESETS = {"sobel_x": 0, "sobel_y": 1, "sobel_mag": 2, "scharr_x": 3, "scharr_y": 4, "scharr_mag": 5,
                "laplacian4": 6, "laplacian8": 7, "sharpen": 8, "emboss": 9}
DECIMATE_MAX = 4
DOWN_PYR, DOWN_AREA2, DOWN_AREA4 = 0, 1, 2
RESIZE_MAX_DIM = 32768
RESIZE_NEAREST, RESIZE_BILINEAR = 0, 1
RESIZE_MODES = {"nearest": RESIZE_NEAREST, "bilinear": RESIZE_BILINEAR}
AREA_MAX_RATIO = 64
COLOR_MAX_CHANNELS = 4
COLOR_CODES = {"rgb2gray": 0, "bgr2gray": 1, "gray2rgb": 2, "rgb2bgr": 3, "rgba2bgra": 4, "rgba2rgb": 5, "rgb2rgba": 6,
               "rgb2ycbcr": 7, "ycbcr2rgb": 8}
HIST_BINS = 256
CLAHE_MAX_TILES = 64
TONE_EQUALIZE, TONE_STRETCH = 0, 1
TONE_MODES = {"equalize": TONE_EQUALIZE, "stretch": TONE_STRETCH}
ARITH_LINEAR, ARITH_ABSDIFF, ARITH_MIN, ARITH_MAX, ARITH_MUL, ARITH_LERP = range(6)
BOX_MEAN, BOX_STDDEV, BOX_THRESHOLD = range(3)
BOX_MAX_RADIUS = 127
DIST_L2, DIST_L1, DIST_LINF = range(3)
DIST_METRICS = {"l2": DIST_L2, "l1": DIST_L1, "linf": DIST_LINF}
DIST_BYTE, DIST_WITHIN = 0, 1
DIST_MAX_LIMIT = 32767
DIST_NONE = 0xFFFFFFFF
MATCH_SQDIFF, MATCH_CCORR, MATCH_SAD, MATCH_NCC, MATCH_ZNCC = range(5)
MATCH_METHODS = {"sqdiff": MATCH_SQDIFF, "ccorr": MATCH_CCORR, "sad": MATCH_SAD, "ncc": MATCH_NCC, "zncc": MATCH_ZNCC}
MATCH_MAX_SIDE, MATCH_MAX_AREA, MATCH_ONE = 255, 65536, 16384
MATCH_PEAK_PARTS = 256
ARITH_PRESETS = {"add": 0, "sub": 1, "avg": 2, "diff128": 3, "absdiff": 4, "min": 5, "max": 6, "mul255": 7, "mulq7": 8, "lerp": 9}
WARP_Q = 16
WARP_CLAMP, WARP_CONSTANT = 0, 1
WARP_BORDERS = {"clamp": WARP_CLAMP, "constant": WARP_CONSTANT}
PEER_HANDLE_BYTES = 64


def _newer(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def build_native(force: bool = False, verbose: bool = False) -> str:
    """Compile libmi_blur.so (hipcc, --offload-arch=gfx950) and the C++ hosts, in-tree."""
    srcs = [os.path.join(CSRC, f) for f in ("blur_kernels.hip", "sep_kernels.hip", "median_kernels.hip", "morph_kernels.hip", "bilateral_kernels.hip", "conv_kernels.hip", "sep_down_kernels.hip", "resize_kernels.hip", "warp_kernels.hip", "remap_kernels.hip", "area_kernels.hip", "color_kernels.hip", "hist_kernels.hip", "clahe_kernels.hip", "arith_kernels.hip", "integral_kernels.hip", "dist_kernels.hip", "match_kernels.hip", "layout_kernels.hip", "mi_blur_api.cpp", "table_api.cpp", "comm_api.cpp", "cpu_device.cpp")]
    deps = srcs + [os.path.join(CSRC, f) for f in ("api_internal.h", "blur_launch.h", "kernel_common.h", "cpu_device.h", "filter.h")] + [HEADER]
    if force or not _newer(LIB_PATH, deps):
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra",
               "-o", LIB_PATH] + srcs + ["-ldl", "-lpthread"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    if os.path.isdir(APPS):
        for app in ("heterogeneous_blur", "split_image_blur"):
            src = os.path.join(APPS, app + ".cpp")
            exe = os.path.join(APPS, app)
            common = [os.path.join(APPS, f) for f in os.listdir(APPS) if f.endswith((".h", ".hpp"))]
            if os.path.exists(src) and (force or not _newer(exe, [src, LIB_PATH, HEADER] + common)):
                cmd = [HIPCC, "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                       "-L", PKG_DIR, "-lmi_blur", f"-Wl,-rpath,$ORIGIN/..", "-lpthread"]
                if verbose:
                    print(" ".join(cmd), flush=True)
                subprocess.run(cmd, check=True)
    return LIB_PATH


def declared_symbols() -> list[str]:
    """Every function include/mi_blur.h declares."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mi_blur_[a-z0-9_]+)\s*\(", text)))


class Timing(C.Structure):
    _fields_ = [("h2d_ms", C.c_double), ("kernel_ms", C.c_double), ("d2h_ms", C.c_double),
                ("bytes_h2d", C.c_uint64), ("bytes_d2h", C.c_uint64), ("bytes_alg", C.c_uint64),
                ("images", C.c_uint64), ("launches", C.c_uint64)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


class A2Geometry(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("split_row", "cpu_input_rows", "cpu_output_rows", "gpu_input_rows", "gpu_output_rows")]


class Band(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("row_begin", "row_end", "halo_top", "halo_bottom")]


class SepKernel(C.Structure):
    """mi_blur_sep_kernel: per axis a radius (0..16), 2r+1 taps summing to 2^b (b <= 8)."""
    _fields_ = [("rx", C.c_int), ("ry", C.c_int), ("bx", C.c_int), ("by", C.c_int),
                ("wx", C.c_uint16 * (2 * SEP_MAX_RADIUS + 1)), ("wy", C.c_uint16 * (2 * SEP_MAX_RADIUS + 1))]

    @classmethod
    def from_taps(cls, wx, wy=None) -> "SepKernel":
        """Taps per axis (sequences of odd length <= 33, each summing to a power of two <= 256); wy None = wx."""
        wy = wx if wy is None else wy
        k = cls()
        for axis, taps in (("x", list(wx)), ("y", list(wy))):
            n, total = len(taps), int(sum(taps))
            if n % 2 != 1 or n > 2 * SEP_MAX_RADIUS + 1 or total <= 0 or total & (total - 1):
                raise ValueError(f"taps {axis}: odd length <= {2 * SEP_MAX_RADIUS + 1}, summing to a power of two")
            setattr(k, "r" + axis, n // 2)
            setattr(k, "b" + axis, total.bit_length() - 1)
            arr = getattr(k, "w" + axis)
            for i, t in enumerate(taps):
                arr[i] = int(t)
        return k

    def taps(self) -> tuple[list[int], list[int]]:
        return list(self.wx[:2 * self.rx + 1]), list(self.wy[:2 * self.ry + 1])


class Bilateral(C.Structure):
    """mi_blur_bilateral: a radius r (1..8), the spatial table S over the (2r+1) x (2r+1) window (row-major at the front of
    `spatial`) and the range table R over |neighbour - centre|."""
    _fields_ = [("radius", C.c_int), ("spatial", C.c_uint8 * (17 * 17)), ("range", C.c_uint8 * 256)]

    @classmethod
    def from_tables(cls, spatial_2d, range_256) -> "Bilateral":
        """spatial_2d: (2r+1) rows of (2r+1) weights 0..255, r in 1..8; range_256: 256 weights 0..255.  The library
        validates the rest (centre and R[0] non-zero, sum S <= 65535) when the kernel is used."""
        rows = [list(row) for row in spatial_2d]
        n = len(rows)
        rng = list(range_256)
        if n % 2 != 1 or not 3 <= n <= 2 * BILATERAL_MAX_RADIUS + 1 or any(len(row) != n for row in rows):
            raise ValueError(f"Bilateral.from_tables: spatial_2d is square with an odd side, 3..{2 * BILATERAL_MAX_RADIUS + 1}")
        if len(rng) != 256:
            raise ValueError("Bilateral.from_tables: range_256 has 256 entries")
        flat = [int(v) for row in rows for v in row]
        rng = [int(v) for v in rng]
        if any(not 0 <= v <= 255 for v in flat + rng):
            raise ValueError("Bilateral.from_tables: weights are 0..255")
        k = cls()
        k.radius = n // 2
        k.spatial[:n * n] = flat
        k.range[:] = rng
        return k

    @classmethod
    def gauss(cls, sigma_space: float, sigma_range: float, radius: int) -> "Bilateral":
        """Gaussian tables (mi_blur_bilateral_gauss); sigma_space <= 0 means radius / 2."""
        k = cls()
        check(lib().mi_blur_bilateral_gauss(float(sigma_space), float(sigma_range), int(radius), C.byref(k)), "mi_blur_bilateral_gauss")
        return k


class Conv(C.Structure):
    """mi_blur_conv: radii rx, ry (0..7), a mode (CONV_SAT | CONV_ABS | CONV_MAG), a shift (0..16), a bias and the signed
    16-bit taps K (and K2 for CONV_MAG), row-major at the front of `k` / `k2`.  Correlation: no flip."""
    _fields_ = [("rx", C.c_int), ("ry", C.c_int), ("mode", C.c_int), ("shift", C.c_int), ("bias", C.c_int32),
                ("k", C.c_int16 * (15 * 15)), ("k2", C.c_int16 * (15 * 15))]

    @classmethod
    def from_taps(cls, kernel_2d, shift: int = 0, bias: int = 0, mode="sat", kernel2_2d=None) -> "Conv":
        """kernel_2d: (2 ry + 1) rows of (2 rx + 1) integer taps, radii 0..7; kernel2_2d (mode "mag" only): the second
        table, same shape.  mode: "sat" | "abs" | "mag" or a CONV_* value.  The library validates the rest (shift, bias,
        sum |K| <= 65535) when the kernel is used."""
        m = CONV_MODES.get(mode, mode) if isinstance(mode, str) else mode
        if m not in (CONV_SAT, CONV_ABS, CONV_MAG):
            raise ValueError('Conv.from_taps: mode is "sat", "abs" or "mag"')
        if (kernel2_2d is not None) != (m == CONV_MAG):
            raise ValueError('Conv.from_taps: kernel2_2d goes with mode "mag", and only with it')
        k = cls()
        shape = None
        for name, table in (("k", kernel_2d), ("k2", kernel2_2d)):
            if table is None:
                continue
            rows = [list(row) for row in table]
            ny, nx = len(rows), len(rows[0]) if rows else 0
            if ny % 2 != 1 or nx % 2 != 1 or ny > 2 * CONV_MAX_RADIUS + 1 or nx > 2 * CONV_MAX_RADIUS + 1 or any(len(r) != nx for r in rows):
                raise ValueError(f"Conv.from_taps: a table has odd sides, 1..{2 * CONV_MAX_RADIUS + 1}")
            if shape is not None and shape != (ny, nx):
                raise ValueError("Conv.from_taps: kernel2_2d has the shape of kernel_2d")
            shape = (ny, nx)
            raw = [v for row in rows for v in row]
            flat = [int(v) for v in raw]
            if any(f != v for f, v in zip(flat, raw)) or any(not -32768 <= f <= 32767 for f in flat):
                raise ValueError("Conv.from_taps: taps are integers -32768..32767")
            getattr(k, name)[:nx * ny] = flat
        k.ry, k.rx = shape[0] // 2, shape[1] // 2
        k.mode, k.shift, k.bias = int(m), int(shift), int(bias)
        return k

    @classmethod
    def preset(cls, name: str) -> "Conv":
        """A ready 3x3 kernel (mi_blur_conv_preset): one of CONV_PRESETS' names."""
        if name not in CONV_PRESETS:
            raise ValueError(f"Conv.preset: one of {sorted(CONV_PRESETS)}")
        k = cls()
        check(lib().mi_blur_conv_preset(CONV_PRESETS[name], C.byref(k)), "mi_blur_conv_preset")
        return k

    def taps(self):
        """(K, K2) as lists of rows; K2 is None unless the mode is CONV_MAG."""
        nx, ny = 2 * self.rx + 1, 2 * self.ry + 1
        t = lambda a: [list(a[j * nx:(j + 1) * nx]) for j in range(ny)]
        return t(self.k), t(self.k2) if self.mode == CONV_MAG else None


class Decimation(C.Structure):
    """mi_blur_decimation: keep column ox + X*sx and row oy + Y*sy (strides 1..4, phases below them)."""
    _fields_ = [("sx", C.c_int), ("sy", C.c_int), ("ox", C.c_int), ("oy", C.c_int)]


class Resize(C.Structure):
    """mi_blur_resize: the output size and the mode (RESIZE_NEAREST | RESIZE_BILINEAR)."""
    _fields_ = [("out_width", C.c_int), ("out_height", C.c_int), ("mode", C.c_int)]


class Area(C.Structure):
    """mi_blur_area: the output size of the area resize."""
    _fields_ = [("out_width", C.c_int), ("out_height", C.c_int)]


class Color(C.Structure):
    """mi_blur_color: out_channels, the shift, the matrix m[o][i], the bias per output channel, and the tables lut[o][v]
    that are read when lut_on."""
    _fields_ = [("out_channels", C.c_int), ("shift", C.c_int), ("m", (C.c_int32 * 4) * 4), ("bias", C.c_int32 * 4),
                ("lut_on", C.c_int), ("lut", (C.c_uint8 * 256) * 4)]


class Tone(C.Structure):
    """mi_blur_tone: the mode, the two clips (Q16 shares, STRETCH only), joint and the channel mask (0 = all)."""
    _fields_ = [("mode", C.c_int), ("clip_lo", C.c_int), ("clip_hi", C.c_int), ("joint", C.c_int), ("channel_mask", C.c_int)]


class Clahe(C.Structure):
    """mi_blur_clahe: the tile grid, the clip limit in Q8 (0 = none) and the channel mask (0 = all)."""
    _fields_ = [("tiles_x", C.c_int), ("tiles_y", C.c_int), ("clip_q8", C.c_int), ("channel_mask", C.c_int)]


class Arith(C.Structure):
    """mi_blur_arith: the operation (ARITH_*), its weights wa, wb, bias and shift, and the plane / shared flags of B and
    of the mask (include/mi_blur.h, "Two-image arithmetic")."""
    _fields_ = [("op", C.c_int), ("wa", C.c_int32), ("wb", C.c_int32), ("bias", C.c_int32), ("shift", C.c_int),
                ("b_plane", C.c_int), ("b_shared", C.c_int), ("m_plane", C.c_int), ("m_shared", C.c_int)]


class Box(C.Structure):
    """mi_blur_box: the operation (BOX_MEAN | BOX_STDDEV | BOX_THRESHOLD), the radii of the (2 rx + 1) x (2 ry + 1) window
    and, for BOX_THRESHOLD only, the offset (-255..255) and invert (include/mi_blur.h, "Integral images, and box filters")."""
    _fields_ = [("op", C.c_int), ("rx", C.c_int), ("ry", C.c_int), ("offset", C.c_int), ("invert", C.c_int)]


class Dist(C.Structure):
    """mi_blur_dist: the metric (DIST_L2 | DIST_L1 | DIST_LINF), whether a site is a non-zero pixel (0: a zero pixel), the
    limit (0 = none, 1..32767) and, for the byte calls, byte_op (DIST_BYTE | DIST_WITHIN) and, for DIST_WITHIN only, invert
    (include/mi_blur.h, "Exact distance transform")."""
    _fields_ = [("metric", C.c_int), ("sites_nonzero", C.c_int), ("limit", C.c_int), ("byte_op", C.c_int), ("invert", C.c_int)]


class Match(C.Structure):
    """mi_blur_match: the method (MATCH_SQDIFF | MATCH_CCORR | MATCH_SAD | MATCH_NCC | MATCH_ZNCC), the template's size and
    whether one template serves every image (include/mi_blur.h, "Template matching and peak search")."""
    _fields_ = [("method", C.c_int), ("tw", C.c_int), ("th", C.c_int), ("t_shared", C.c_int)]


class Warp(C.Structure):
    """mi_blur_warp: the output size, the mode (RESIZE_NEAREST | RESIZE_BILINEAR), the border (WARP_CLAMP | WARP_CONSTANT),
    the fill byte and the OUTPUT -> INPUT map in Q16, row-major 2 x 3."""
    _fields_ = [("out_width", C.c_int), ("out_height", C.c_int), ("mode", C.c_int), ("border", C.c_int), ("fill", C.c_int),
                ("m", C.c_int64 * 6)]

    @classmethod
    def from_matrix(cls, M, out_width: int, out_height: int, mode="bilinear", border="constant", fill: int = 0, inverse: bool = False) -> "Warp":
        """M: a real 2 x 3 matrix, input -> output (inverse=False: what OpenCV's warpAffine takes) or output -> input
        (inverse=True: WARP_INVERSE_MAP); quantised by mi_blur_warp_set_matrix."""
        w = cls(int(out_width), int(out_height), _resize_mode(mode, "warp_affine"), _warp_border(border), int(fill))
        flat = [float(v) for row in M for v in (row if hasattr(row, "__len__") else [row])]
        if len(flat) != 6:
            raise ValueError("warp_affine: M is a 2 x 3 matrix")
        check(lib().mi_blur_warp_set_matrix(C.byref(w), (C.c_double * 6)(*flat), int(bool(inverse))), "mi_blur_warp_set_matrix")
        return w


class WarpPerspective(C.Structure):
    """mi_blur_warp_perspective: the output size, the mode, the border, the fill byte (as Warp) and the OUTPUT -> INPUT
    homography, row-major 3 x 3 int64, free scale."""
    _fields_ = [("out_width", C.c_int), ("out_height", C.c_int), ("mode", C.c_int), ("border", C.c_int), ("fill", C.c_int),
                ("h", C.c_int64 * 9)]

    @classmethod
    def from_matrix(cls, M, out_width: int, out_height: int, mode="bilinear", border="constant", fill: int = 0, inverse: bool = False) -> "WarpPerspective":
        """M: a real 3 x 3 matrix, input -> output (inverse=False: what OpenCV's warpPerspective takes) or output -> input
        (inverse=True: WARP_INVERSE_MAP); normalised and quantised by mi_blur_warp_perspective_set_matrix for this output size."""
        w = cls(int(out_width), int(out_height), _resize_mode(mode, "warp_perspective"), _warp_border(border), int(fill))
        flat = [float(v) for row in M for v in (row if hasattr(row, "__len__") else [row])]
        if len(flat) != 9:
            raise ValueError("warp_perspective: M is a 3 x 3 matrix")
        check(lib().mi_blur_warp_perspective_set_matrix(C.byref(w), (C.c_double * 9)(*flat), int(bool(inverse))), "mi_blur_warp_perspective_set_matrix")
        return w


class Remap(C.Structure):
    """mi_blur_remap: the output size, the mode, the border and the fill byte (as Warp), and stage_bytes: the largest tile
    footprint the tiled kernel stages in LDS (0 = 65520).  The map itself is a separate int32 (Ho, Wo, 2) array."""
    _fields_ = [("out_width", C.c_int), ("out_height", C.c_int), ("mode", C.c_int), ("border", C.c_int), ("fill", C.c_int),
                ("stage_bytes", C.c_int)]


class RemapTiles(C.Structure):
    """mi_blur_remap_tiles: what mi_blur_remap_plan reports."""
    _fields_ = [("tiled", C.c_int), ("tiles", C.c_int), ("staged", C.c_int), ("direct", C.c_int), ("empty", C.c_int),
                ("max_box_bytes", C.c_longlong), ("max_staged_bytes", C.c_longlong)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


def _warp_border(border) -> int:
    if isinstance(border, str):
        if border not in WARP_BORDERS:
            raise ValueError("warp_affine: border is 'constant' or 'clamp'")
        return WARP_BORDERS[border]
    return int(border)


def _resize_mode(mode, name: str = "resize") -> int:
    if isinstance(mode, str):
        if mode not in RESIZE_MODES:
            raise ValueError(f"{name}: mode is 'bilinear' or 'nearest'")
        return RESIZE_MODES[mode]
    return int(mode)


class MiBlurError(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: status {status} ({lib().mi_blur_strerror(status).decode()})")
        self.status = status


_lib = None


def lib() -> C.CDLL:
    """Load libmi_blur.so (raises if it has not been built — there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    # torch wheels bundle their own libamdhip64/libhsa-runtime64 and load them by path.  If this
    # library were loaded first it would pull /opt/rocm's copies in and the process would hold
    # TWO HIP runtimes fighting over the device (measured: device count 0 / torch unavailable).
    # Harness processes use torch for device memory, so load torch first: libmi_blur.so then binds
    # to the already-loaded runtime by soname.  (The C++ hosts never load torch: one runtime.)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i, u8p = C.c_void_p, C.c_int, C.c_void_p
    sig = {
        "mi_blur_strerror": (C.c_char_p, [i]),
        "mi_blur_version": (i, []),
        "mi_blur_last_kernel": (C.c_char_p, []),
        "mi_blur_device_count": (i, []),
        "mi_blur_set_option": (i, [C.c_char_p, i]),
        "mi_blur_enqueue": (i, [u8p, u8p, i, i, i, i, i, vp]),
        "mi_blur_enqueue_band": (i, [u8p, u8p, i, i, i, i, i, i, vp]),
        "mi_blur_enqueue_ex": (i, [u8p, u8p, i, i, i, i, i, i, i, i, vp]),
        "mi_blur_planar_to_interleaved": (i, [u8p, u8p, i, i, i, i, vp]),
        "mi_blur_interleaved_to_planar": (i, [u8p, u8p, i, i, i, i, vp]),
        "mi_blur_create": (i, [C.POINTER(vp), i, i, i, i, i, i, i, i]),
        "mi_blur_destroy": (None, [vp]),
        "mi_blur_host_alloc": (vp, [C.c_size_t]),
        "mi_blur_host_free": (None, [vp]),
        "mi_blur_host_register": (i, [vp, C.c_size_t]),
        "mi_blur_host_unregister": (i, [vp]),
        "mi_blur_device_cpulist": (i, [i, C.c_char_p, C.c_size_t, C.POINTER(i)]),
        "mi_blur_bind_thread_to_device": (i, [i]),
        "mi_blur_host_alloc_on": (vp, [i, C.c_size_t]),
        "mi_blur_submit": (i, [vp, u8p, u8p, i]),
        "mi_blur_submit_band": (i, [vp, u8p, u8p, i, i, i]),
        "mi_blur_submit_bands": (i, [vp, u8p, u8p, i, C.c_size_t, i, i, i]),
        "mi_blur_submit_planar": (i, [vp, u8p, u8p, i, i]),
        "mi_blur_wait_oldest": (i, [vp]),
        "mi_blur_sync": (i, [vp, C.POINTER(Timing)]),
        "mi_blur_reset_timing": (None, [vp]),
        "mi_blur_get_timing": (C.c_int, [vp, C.c_void_p]),
        "mi_blur_resident_run_fused": (C.c_int, [vp, C.c_int, C.c_int, C.c_int]),
        "mi_blur_resident_batches_done": (C.c_int, [vp]),
        "mi_blur_resident_peek": (C.c_int, [vp, C.c_int, u8p, C.c_int]),
        "mi_blur_zero_copy_launches": (C.c_uint64, [vp]),
        "mi_blur_resident_alloc": (i, [vp, i]),
        "mi_blur_resident_placement": (i, [vp, C.POINTER(C.c_float), i, C.POINTER(i)]),
        "mi_blur_resident_fill_synthetic": (i, [vp, i]),
        "mi_blur_resident_upload": (i, [vp, i, u8p, i]),
        "mi_blur_resident_download": (i, [vp, i, u8p, i]),
        "mi_blur_resident_in": (vp, [vp]),
        "mi_blur_resident_out": (vp, [vp]),
        "mi_blur_resident_run": (i, [vp, i, i, i]),
        "mi_blur_timed_coverage": (None, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "mi_blur_cpu_run": (i, [u8p, u8p, i, i, i, i, i, i]),
        "mi_blur_gauss_taps": (i, [C.c_double, i, i, C.POINTER(C.c_uint16), C.POINTER(i)]),
        "mi_blur_sep_kernel_gauss": (i, [C.c_double, C.c_double, i, i, C.POINTER(SepKernel)]),
        "mi_blur_enqueue_sep": (i, [u8p, u8p, i, i, i, i, C.POINTER(SepKernel), vp]),
        "mi_blur_enqueue_sep_band": (i, [u8p, u8p, i, i, i, i, i, C.POINTER(SepKernel), vp]),
        "mi_blur_cpu_run_sep": (i, [u8p, u8p, i, i, i, i, C.POINTER(SepKernel), i]),
        "mi_blur_ctx_set_kernel": (i, [vp, C.POINTER(SepKernel)]),
        "mi_blur_enqueue_median": (i, [u8p, u8p, i, i, i, i, i, vp]),
        "mi_blur_enqueue_median_band": (i, [u8p, u8p, i, i, i, i, i, i, vp]),
        "mi_blur_cpu_run_median": (i, [u8p, u8p, i, i, i, i, i, i]),
        "mi_blur_ctx_set_median": (i, [vp, i]),
        "mi_blur_enqueue_morph": (i, [u8p, u8p, i, i, i, i, i, i, i, vp]),
        "mi_blur_enqueue_morph_band": (i, [u8p, u8p, i, i, i, i, i, i, i, i, vp]),
        "mi_blur_cpu_run_morph": (i, [u8p, u8p, i, i, i, i, i, i, i, i]),
        "mi_blur_ctx_set_morph": (i, [vp, i, i, i]),
        "mi_blur_bilateral_gauss": (i, [C.c_double, C.c_double, i, C.POINTER(Bilateral)]),
        "mi_blur_enqueue_bilateral": (i, [u8p, u8p, i, i, i, i, C.POINTER(Bilateral), vp]),
        "mi_blur_enqueue_bilateral_band": (i, [u8p, u8p, i, i, i, i, i, C.POINTER(Bilateral), vp]),
        "mi_blur_cpu_run_bilateral": (i, [u8p, u8p, i, i, i, i, C.POINTER(Bilateral), i]),
        "mi_blur_ctx_set_bilateral": (i, [vp, C.POINTER(Bilateral)]),
        "mi_blur_decimated_size": (i, [i, i, C.POINTER(Decimation), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_sep_down_preset": (i, [i, C.POINTER(SepKernel), C.POINTER(Decimation)]),
        "mi_blur_enqueue_sep_down": (i, [u8p, u8p, i, i, i, i, C.POINTER(SepKernel), C.POINTER(Decimation), vp]),
        "mi_blur_cpu_run_sep_down": (i, [u8p, u8p, i, i, i, i, C.POINTER(SepKernel), C.POINTER(Decimation), i]),
        "mi_blur_ctx_set_sep_down": (i, [vp, C.POINTER(SepKernel), C.POINTER(Decimation)]),
        "mi_blur_resize_coord": (i, [i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_enqueue_resize": (i, [u8p, u8p, i, i, i, i, C.POINTER(Resize), vp]),
        "mi_blur_cpu_run_resize": (i, [u8p, u8p, i, i, i, i, C.POINTER(Resize), i]),
        "mi_blur_ctx_set_resize": (i, [vp, C.POINTER(Resize)]),
        "mi_blur_area_coord": (i, [i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_enqueue_area": (i, [u8p, u8p, i, i, i, i, C.POINTER(Area), vp]),
        "mi_blur_cpu_run_area": (i, [u8p, u8p, i, i, i, i, C.POINTER(Area), i]),
        "mi_blur_ctx_set_area": (i, [vp, C.POINTER(Area)]),
        "mi_blur_color_preset": (i, [i, C.POINTER(Color)]),
        "mi_blur_color_identity": (i, [i, C.POINTER(Color)]),
        "mi_blur_color_lut_gamma": (i, [C.c_double, u8p]),
        "mi_blur_color_lut_threshold": (i, [i, i, i, u8p]),
        "mi_blur_enqueue_color": (i, [u8p, u8p, i, i, i, i, C.POINTER(Color), vp]),
        "mi_blur_cpu_run_color": (i, [u8p, u8p, i, i, i, i, C.POINTER(Color), i]),
        "mi_blur_ctx_set_color": (i, [vp, C.POINTER(Color)]),
        "mi_blur_enqueue_hist": (i, [u8p, vp, i, i, i, i, vp]),
        "mi_blur_cpu_run_hist": (i, [u8p, vp, i, i, i, i, i]),
        "mi_blur_tone_tables": (i, [vp, i, C.POINTER(Tone), u8p]),
        "mi_blur_enqueue_tables": (i, [u8p, u8p, i, i, i, i, u8p, vp]),
        "mi_blur_tone_work_bytes": (C.c_size_t, [i, i]),
        "mi_blur_enqueue_tone": (i, [u8p, u8p, i, i, i, i, C.POINTER(Tone), vp, vp]),
        "mi_blur_cpu_run_tables": (i, [u8p, u8p, i, i, i, i, u8p, i]),
        "mi_blur_cpu_run_tone": (i, [u8p, u8p, i, i, i, i, C.POINTER(Tone), vp, i]),
        "mi_blur_run_hist": (i, [i, u8p, vp, i, i, i, i]),
        "mi_blur_run_tone": (i, [i, u8p, u8p, vp, i, i, i, i, C.POINTER(Tone)]),
        "mi_blur_clahe_coord": (i, [i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_clahe_table": (i, [vp, C.c_uint32, i, u8p]),
        "mi_blur_clahe_work_bytes": (C.c_size_t, [i, i, i, i, C.POINTER(Clahe)]),
        "mi_blur_enqueue_clahe_tables": (i, [u8p, i, i, i, i, C.POINTER(Clahe), vp, vp]),
        "mi_blur_enqueue_clahe_apply": (i, [u8p, u8p, i, i, i, i, C.POINTER(Clahe), u8p, vp]),
        "mi_blur_enqueue_clahe": (i, [u8p, u8p, i, i, i, i, C.POINTER(Clahe), vp, vp]),
        "mi_blur_cpu_run_clahe_tables": (i, [u8p, i, i, i, i, C.POINTER(Clahe), vp, i]),
        "mi_blur_cpu_run_clahe_apply": (i, [u8p, u8p, i, i, i, i, C.POINTER(Clahe), u8p, i]),
        "mi_blur_cpu_run_clahe": (i, [u8p, u8p, i, i, i, i, C.POINTER(Clahe), vp, i]),
        "mi_blur_run_clahe": (i, [i, u8p, u8p, vp, i, i, i, i, C.POINTER(Clahe)]),
        "mi_blur_arith_preset": (i, [i, C.POINTER(Arith)]),
        "mi_blur_arith_weighted": (i, [C.c_double, C.c_double, C.c_double, C.POINTER(Arith)]),
        "mi_blur_arith_value": (i, [C.POINTER(Arith), i, i, i]),
        "mi_blur_enqueue_arith": (i, [u8p, u8p, u8p, u8p, i, i, i, i, C.POINTER(Arith), vp]),
        "mi_blur_cpu_run_arith": (i, [u8p, u8p, u8p, u8p, i, i, i, i, C.POINTER(Arith), i]),
        "mi_blur_run_arith": (i, [i, u8p, u8p, u8p, u8p, i, i, i, i, C.POINTER(Arith)]),
        "mi_blur_box_value": (i, [C.POINTER(Box), i, C.c_uint32, C.c_uint32, i]),
        "mi_blur_integral_work_bytes": (C.c_size_t, [i, i, i, i, i]),
        "mi_blur_enqueue_integral": (i, [u8p, vp, vp, i, i, i, i, vp, vp]),
        "mi_blur_cpu_run_integral": (i, [u8p, vp, vp, i, i, i, i, i]),
        "mi_blur_enqueue_box_from_integral": (i, [u8p, vp, vp, u8p, i, i, i, i, C.POINTER(Box), vp]),
        "mi_blur_box_work_bytes": (C.c_size_t, [i, i, i, i, C.POINTER(Box)]),
        "mi_blur_enqueue_box": (i, [u8p, u8p, i, i, i, i, C.POINTER(Box), vp, vp]),
        "mi_blur_cpu_run_box": (i, [u8p, u8p, i, i, i, i, C.POINTER(Box), i]),
        "mi_blur_run_integral": (i, [i, u8p, vp, vp, i, i, i, i]),
        "mi_blur_run_box": (i, [i, u8p, u8p, i, i, i, i, C.POINTER(Box)]),
        "mi_blur_dist_value": (i, [C.POINTER(Dist), C.c_uint32]),
        "mi_blur_dist_work_bytes": (C.c_size_t, [i, i, i, i, C.POINTER(Dist)]),
        "mi_blur_enqueue_dist": (i, [u8p, vp, i, i, i, i, C.POINTER(Dist), vp, vp]),
        "mi_blur_enqueue_dist_u8": (i, [u8p, u8p, i, i, i, i, C.POINTER(Dist), vp, vp]),
        "mi_blur_cpu_run_dist": (i, [u8p, vp, i, i, i, i, C.POINTER(Dist), i]),
        "mi_blur_cpu_run_dist_u8": (i, [u8p, u8p, i, i, i, i, C.POINTER(Dist), i]),
        "mi_blur_run_dist": (i, [i, u8p, vp, i, i, i, i, C.POINTER(Dist)]),
        "mi_blur_run_dist_u8": (i, [i, u8p, u8p, i, i, i, i, C.POINTER(Dist)]),
        "mi_blur_match_value": (C.c_int32, [i, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
        "mi_blur_match_work_bytes": (C.c_size_t, [i, i, i, i, C.POINTER(Match)]),
        "mi_blur_enqueue_match": (i, [u8p, u8p, vp, i, i, i, i, C.POINTER(Match), vp, vp]),
        "mi_blur_cpu_run_match": (i, [u8p, u8p, vp, i, i, i, i, C.POINTER(Match), i]),
        "mi_blur_run_match": (i, [i, u8p, u8p, vp, i, i, i, i, C.POINTER(Match)]),
        "mi_blur_match_peak_work_bytes": (C.c_size_t, [i, i, i]),
        "mi_blur_enqueue_match_peak": (i, [vp, i, i, i, i, vp, vp, vp]),
        "mi_blur_cpu_run_match_peak": (i, [vp, i, i, i, i, vp, i]),
        "mi_blur_run_match_peak": (i, [i, vp, i, i, i, i, vp]),
        "mi_blur_warp_coord": (i, [C.POINTER(Warp), i, i, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_warp_rotation": (i, [C.c_double, C.c_double, C.c_double, C.c_double, C.POINTER(C.c_double)]),
        "mi_blur_warp_set_matrix": (i, [C.POINTER(Warp), C.POINTER(C.c_double), i]),
        "mi_blur_enqueue_warp": (i, [u8p, u8p, i, i, i, i, C.POINTER(Warp), vp]),
        "mi_blur_cpu_run_warp": (i, [u8p, u8p, i, i, i, i, C.POINTER(Warp), i]),
        "mi_blur_ctx_set_warp": (i, [vp, C.POINTER(Warp)]),
        "mi_blur_warp_perspective_coord": (i, [C.POINTER(WarpPerspective), i, i, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_warp_perspective_quad": (i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
        "mi_blur_warp_perspective_set_matrix": (i, [C.POINTER(WarpPerspective), C.POINTER(C.c_double), i]),
        "mi_blur_enqueue_warp_perspective": (i, [u8p, u8p, i, i, i, i, C.POINTER(WarpPerspective), vp]),
        "mi_blur_cpu_run_warp_perspective": (i, [u8p, u8p, i, i, i, i, C.POINTER(WarpPerspective), i]),
        "mi_blur_ctx_set_warp_perspective": (i, [vp, C.POINTER(WarpPerspective)]),
        "mi_blur_remap_coord": (i, [C.POINTER(Remap), i, i, C.c_int32, C.c_int32, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_remap_from_float": (i, [vp, vp, C.c_size_t, vp]),
        "mi_blur_remap_undistort": (i, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), i, i, vp]),
        "mi_blur_remap_plan": (i, [vp, i, i, i, C.POINTER(Remap), C.POINTER(RemapTiles)]),
        "mi_blur_enqueue_remap": (i, [u8p, u8p, i, i, i, i, C.POINTER(Remap), vp, vp]),
        "mi_blur_cpu_run_remap": (i, [u8p, u8p, i, i, i, i, C.POINTER(Remap), vp, i]),
        "mi_blur_ctx_set_remap": (i, [vp, C.POINTER(Remap), vp]),
        "mi_blur_conv_preset": (i, [i, C.POINTER(Conv)]),
        "mi_blur_enqueue_conv": (i, [u8p, u8p, i, i, i, i, C.POINTER(Conv), vp]),
        "mi_blur_enqueue_conv_band": (i, [u8p, u8p, i, i, i, i, i, C.POINTER(Conv), vp]),
        "mi_blur_cpu_run_conv": (i, [u8p, u8p, i, i, i, i, C.POINTER(Conv), i]),
        "mi_blur_ctx_set_conv": (i, [vp, C.POINTER(Conv)]),
        "mi_blur_fill_synthetic": (None, [u8p, i, i, i, i, i, i]),
        "mi_blur_fnv1a64": (C.c_uint64, [u8p, C.c_size_t]),
        "mi_blur_debug_zc_trace": (i, [vp, C.POINTER(C.c_uint64), i, C.POINTER(i), C.POINTER(C.c_uint)]),
        "mi_blur_debug_xcd_times": (i, [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), i]),
        "mi_blur_debug_xcd_raw": (i, [C.POINTER(C.c_uint64), C.c_size_t, C.c_size_t]),
        "mi_blur_a1_partition": (None, [i, i, C.c_float, C.POINTER(i), C.POINTER(i)]),
        "mi_blur_shard_range": (None, [C.c_longlong, i, i, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
        "mi_blur_a2_split": (None, [i, C.c_float, i, C.POINTER(A2Geometry)]),
        "mi_blur_band_of": (None, [i, i, i, i, C.POINTER(Band)]),
        "mi_blur_comm_unique_id": (i, [vp]),
        "mi_blur_comm_init_rank": (i, [C.POINTER(vp), i, i, vp]),
        "mi_blur_comm_init_all": (i, [C.POINTER(vp), i, C.POINTER(i)]),
        "mi_blur_comm_init_p2p": (i, [C.POINTER(vp), i, C.POINTER(i)]),
        "mi_blur_comm_init_pull": (i, [C.POINTER(vp), i, C.POINTER(i)]),
        "mi_blur_comm_destroy": (None, [vp]),
        "mi_blur_comm_info": (i, [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "mi_blur_halo_exchange": (i, [vp, u8p, i, i, i, i, vp]),
        "mi_blur_peer_export": (i, [vp, vp, C.POINTER(C.c_uint64)]),
        "mi_blur_peer_open": (i, [vp, C.c_uint64, C.POINTER(vp)]),
        "mi_blur_peer_close": (i, [vp, C.c_uint64]),
        "mi_blur_halo_pull": (i, [u8p, u8p, u8p, i, i, i, i, vp]),
        "mi_blur_enqueue_band_peer": (i, [u8p, u8p, i, i, i, i, i, i, u8p, u8p, vp]),
        "mi_blur_halo_exchange_all": (i, [C.POINTER(vp), i, C.POINTER(vp), i, i, C.POINTER(i), i, C.POINTER(vp)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)      # AttributeError if the library does not export it
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


def check(status: int, what: str = "mi_blur") -> None:
    if status != OK:
        raise MiBlurError(status, what)


# ---- thin conveniences over the ABI (no logic beyond argument marshalling) -----------------
def a1_partition(mode: int, batch_count: int, gpu_ratio: float) -> tuple[int, int]:
    nc, ng = C.c_int(), C.c_int()
    lib().mi_blur_a1_partition(mode, batch_count, gpu_ratio, C.byref(nc), C.byref(ng))
    return nc.value, ng.value


def shard_range(n_units: int, g: int, G: int) -> tuple[int, int]:
    b, e = C.c_longlong(), C.c_longlong()
    lib().mi_blur_shard_range(n_units, g, G, C.byref(b), C.byref(e))
    return b.value, e.value


def device_cpulist(device: int) -> tuple[str, int]:
    """(local CPU list as sysfs spells it, NUMA node) of a GPU; ("", -1) when the topology is not exposed."""
    buf = C.create_string_buffer(512)
    node = C.c_int(-1)
    rc = lib().mi_blur_device_cpulist(device, buf, len(buf), C.byref(node))
    return (buf.value.decode() if rc == OK else "", node.value)


def gauss_taps(sigma: float, radius: int = 0, bits: int = 8) -> list[int]:
    """Integer Gaussian taps (mi_blur_gauss_taps): 2r'+1 values summing to 2^bits, r' the trimmed radius."""
    taps = (C.c_uint16 * (2 * SEP_MAX_RADIUS + 1))()
    r = C.c_int()
    check(lib().mi_blur_gauss_taps(float(sigma), int(radius), int(bits), taps, C.byref(r)), "mi_blur_gauss_taps")
    return list(taps[:2 * r.value + 1])


def gauss_kernel(sigma: float, sigma_y: float | None = None, radius: int = 0, bits: int = 8) -> SepKernel:
    """Both axes (mi_blur_sep_kernel_gauss); sigma_y None = sigma."""
    k = SepKernel()
    check(lib().mi_blur_sep_kernel_gauss(float(sigma), float(sigma_y or 0.0), int(radius), int(bits), C.byref(k)),
          "mi_blur_sep_kernel_gauss")
    return k


def a2_split(height: int, gpu_ratio: float, halo: int = 1) -> dict:
    g = A2Geometry()
    lib().mi_blur_a2_split(height, gpu_ratio, halo, C.byref(g))
    return {n: getattr(g, n) for n, _ in A2Geometry._fields_}


def band_of(height: int, radius: int, g: int, G: int) -> dict:
    b = Band()
    lib().mi_blur_band_of(height, radius, g, G, C.byref(b))
    return {n: getattr(b, n) for n, _ in Band._fields_}


class Context:
    """RAII wrapper of mi_blur_ctx for tests/bench."""

    def __init__(self, device: int, width: int, height: int, channels: int, radius: int = 1,
                 max_batch: int = 1, n_slots: int = 2, n_threads: int = 0):
        self.h = C.c_void_p()
        check(lib().mi_blur_create(C.byref(self.h), device, width, height, channels, radius, max_batch,
                                   n_slots, n_threads), "mi_blur_create")
        self.shape = (height, width, channels)
        self.radius = radius

    def close(self) -> None:
        if self.h:
            lib().mi_blur_destroy(self.h)
            self.h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_median(self, radius: int) -> None:
        """The median of that radius (1..7) in place of the blur, for every submit (before the first one only)."""
        check(lib().mi_blur_ctx_set_median(self.h, int(radius)), "mi_blur_ctx_set_median")
        self.median_radius = int(radius)

    def set_morph(self, op: int, rx: int, ry: int) -> None:
        """Erode / dilate / gradient (MORPH_*) over (2 rx + 1) x (2 ry + 1) in place of the blur (before the first submit only)."""
        check(lib().mi_blur_ctx_set_morph(self.h, int(op), int(rx), int(ry)), "mi_blur_ctx_set_morph")
        self.morph = (int(op), int(rx), int(ry))

    def set_bilateral(self, k: "Bilateral") -> None:
        """The bilateral filter k in place of the blur, for every submit (before the first one only)."""
        check(lib().mi_blur_ctx_set_bilateral(self.h, C.byref(k)), "mi_blur_ctx_set_bilateral")
        self.bilateral = k

    def set_conv(self, k: "Conv") -> None:
        """The signed 2-D convolution k in place of the blur, for every submit (before the first one only)."""
        check(lib().mi_blur_ctx_set_conv(self.h, C.byref(k)), "mi_blur_ctx_set_conv")
        self.conv = k

    def set_kernel(self, kernel: "SepKernel") -> None:
        """A separable kernel in place of the radius, for every submit (before the first one only)."""
        check(lib().mi_blur_ctx_set_kernel(self.h, C.byref(kernel)), "mi_blur_ctx_set_kernel")
        self.kernel = kernel

    def set_sep_down(self, kernel: "SepKernel", sx: int = 2, sy: int = 2, ox: int = 0, oy: int = 0) -> None:
        """The decimating separable filter in place of the blur (before the first submit only): submit() then writes
        images of decimated_size(W, H, sx, sy, ox, oy); the band, planar and resident forms are not supported."""
        d = Decimation(int(sx), int(sy), int(ox), int(oy))
        check(lib().mi_blur_ctx_set_sep_down(self.h, C.byref(kernel), C.byref(d)), "mi_blur_ctx_set_sep_down")
        self.kernel, self.decimation = kernel, d

    def set_resize(self, out_width: int, out_height: int, mode="bilinear") -> None:
        """The resize in place of the blur (before the first submit only): submit() then writes images of
        out_width x out_height, which may be larger than the input; the band, planar and resident forms are not supported."""
        r = Resize(int(out_width), int(out_height), _resize_mode(mode))
        check(lib().mi_blur_ctx_set_resize(self.h, C.byref(r)), "mi_blur_ctx_set_resize")
        self.resize_spec = r

    def set_area(self, out_width: int, out_height: int) -> None:
        """The area resize in place of the blur (before the first submit only): submit() then writes images of
        out_width x out_height; the band, planar and resident forms are not supported."""
        r = Area(int(out_width), int(out_height))
        check(lib().mi_blur_ctx_set_area(self.h, C.byref(r)), "mi_blur_ctx_set_area")
        self.area_spec = r

    def set_color(self, color: "Color") -> None:
        """The colour transform in place of the blur (before the first submit only): submit() then writes images of
        color.out_channels channels; the band, planar and resident forms are not supported."""
        check(lib().mi_blur_ctx_set_color(self.h, C.byref(color)), "mi_blur_ctx_set_color")
        self.color_spec = color

    def set_warp(self, warp: "Warp") -> None:
        """The affine warp in place of the blur (before the first submit only): submit() then writes images of
        warp.out_width x warp.out_height."""
        check(lib().mi_blur_ctx_set_warp(self.h, C.byref(warp)), "mi_blur_ctx_set_warp")
        self.warp_spec = warp

    def set_warp_perspective(self, warp: "WarpPerspective") -> None:
        """The perspective warp in place of the blur (before the first submit only): submit() then writes images of
        warp.out_width x warp.out_height."""
        check(lib().mi_blur_ctx_set_warp_perspective(self.h, C.byref(warp)), "mi_blur_ctx_set_warp_perspective")
        self.warp_spec = warp

    def set_remap(self, remap: "Remap", map) -> None:
        """The remap in place of the blur (before the first submit only): map is an int32 array of shape
        (remap.out_height, remap.out_width, 2), of which the context keeps its own copy; submit() then writes images of
        remap.out_width x remap.out_height."""
        m = _fixed_map(map, "set_remap")
        if m.shape[:2] != (remap.out_height, remap.out_width):
            raise ValueError("set_remap: the map is (out_height, out_width, 2)")
        check(lib().mi_blur_ctx_set_remap(self.h, C.byref(remap), m.ctypes.data), "mi_blur_ctx_set_remap")
        self.remap_spec = remap

    def submit_bands(self, host_in, host_out, n_images: int, host_image_stride: int, band_rows: int,
                     halo_top: int, halo_bottom: int) -> None:
        check(lib().mi_blur_submit_bands(self.h, host_in, host_out, n_images, host_image_stride, band_rows, halo_top,
                                         halo_bottom), "mi_blur_submit_bands")

    def submit(self, host_in, host_out, n_images: int) -> None:
        check(lib().mi_blur_submit(self.h, host_in, host_out, n_images), "mi_blur_submit")

    def submit_band(self, host_in, host_out, band_rows: int, halo_top: int, halo_bottom: int) -> None:
        check(lib().mi_blur_submit_band(self.h, host_in, host_out, band_rows, halo_top, halo_bottom),
              "mi_blur_submit_band")

    def submit_planar(self, host_planar_in, host_out, n_images: int, planar_out: bool = False) -> None:
        check(lib().mi_blur_submit_planar(self.h, host_planar_in, host_out, n_images, 1 if planar_out else 0), "mi_blur_submit_planar")

    def wait_oldest(self) -> None:
        check(lib().mi_blur_wait_oldest(self.h), "mi_blur_wait_oldest")

    def sync(self) -> dict:
        t = Timing()
        check(lib().mi_blur_sync(self.h, C.byref(t)), "mi_blur_sync")
        return t.as_dict()

    def timing(self) -> dict:
        """Non-blocking snapshot of the buckets harvested so far."""
        t = Timing()
        check(lib().mi_blur_get_timing(self.h, C.byref(t)), "mi_blur_get_timing")
        return t.as_dict()

    def reset_timing(self) -> None:
        lib().mi_blur_reset_timing(self.h)

    def resident_alloc(self, pool_images: int) -> None:
        check(lib().mi_blur_resident_alloc(self.h, pool_images), "mi_blur_resident_alloc")

    def resident_placement(self) -> dict:
        """What resident_alloc measured when it chose the pool: per-launch us of each candidate placement, and the one kept."""
        ms = (C.c_float * 64)()
        kept = C.c_int()
        n = lib().mi_blur_resident_placement(self.h, ms, 64, C.byref(kept))
        return {"candidates_us": [round(ms[k] * 1e3, 2) for k in range(max(n, 0))], "kept": kept.value}

    def resident_fill_synthetic(self, first_index: int = 0) -> None:
        check(lib().mi_blur_resident_fill_synthetic(self.h, first_index), "mi_blur_resident_fill_synthetic")

    def resident_upload(self, pool_index: int, host_in, n_images: int) -> None:
        check(lib().mi_blur_resident_upload(self.h, pool_index, host_in, n_images), "mi_blur_resident_upload")

    def resident_download(self, pool_index: int, host_out, n_images: int) -> None:
        check(lib().mi_blur_resident_download(self.h, pool_index, host_out, n_images), "mi_blur_resident_download")

    def resident_run(self, n_images: int, batch: int, timed: int | bool = 0) -> None:
        """timed: 0/False none, 1/True every launch, n every n-th launch carries timestamp events."""
        check(lib().mi_blur_resident_run(self.h, n_images, batch, int(timed)), "mi_blur_resident_run")

    def resident_run_fused(self, n_images: int, batch: int, timed: bool = False, watch: bool = False) -> None:
        """watch: a one-wave kernel keeps the pass's progress in pinned host memory (resident_batches_done then costs no HIP call)."""
        check(lib().mi_blur_resident_run_fused(self.h, n_images, batch, (1 if timed else 0) | (2 if watch else 0)), "mi_blur_resident_run_fused")

    def resident_peek(self, pool_index: int, host_out, n_images: int) -> None:
        check(lib().mi_blur_resident_peek(self.h, pool_index, host_out, n_images), "mi_blur_resident_peek")

    def resident_batches_done(self) -> int:
        """Leading batches of the latest fused pass that are complete; raises on a negative status."""
        n = int(lib().mi_blur_resident_batches_done(self.h))
        if n < 0:
            raise MiBlurError(n, "mi_blur_resident_batches_done")
        return n

    def wait_batches(self, want: int, timeout_s: float = 30.0) -> int:
        """Poll until at least `want` leading batches are done; TimeoutError (with the last count) after timeout_s."""
        import time
        deadline = time.monotonic() + timeout_s
        n = self.resident_batches_done()
        while n < want:
            if time.monotonic() > deadline:
                raise TimeoutError(f"fused stream: {n} of {want} batches counted in after {timeout_s:.0f} s")
            n = self.resident_batches_done()
        return n

    def timed_coverage(self) -> tuple[int, int]:
        n, b = C.c_uint64(), C.c_uint64()
        lib().mi_blur_timed_coverage(self.h, C.byref(n), C.byref(b))
        return n.value, b.value


def _images(images, name: str):
    """images as a contiguous uint8 array of shape (H, W), (H, W, C) or (N, H, W, C); ValueError otherwise."""
    import numpy as np
    a = np.ascontiguousarray(images)
    if a.dtype != np.uint8 or a.ndim not in (2, 3, 4):
        raise ValueError(f"{name}: a uint8 array of shape (H, W), (H, W, C) or (N, H, W, C)")
    return a


def _filter_images(a, radius: int, device: int, batch: int, configure=None, out_size=None, out_channels=None):
    """The numpy driver of every filter function: a (from _images) through mi_blur_create (radius) / configure(ctx) /
    mi_blur_submit / mi_blur_sync.  Returns the output as (N, H, W, C), or as (N, Ho, Wo, C) for a filter whose output
    has a size of its own: out_size = (Ho, Wo), and with out_channels in place of C for one whose output has a channel
    count of its own."""
    import numpy as np
    if a.ndim == 2:
        a = a[None, :, :, None]
    elif a.ndim == 3:
        a = a[None]
    n, h, w, c = a.shape
    ho, wo = out_size or (h, w)
    co = out_channels or c
    out = np.empty((n, ho, wo, co), dtype=np.uint8)
    if n == 0 or a.size == 0:
        return out
    per = min(n, batch if batch > 0 else 4096)
    isz, osz = h * w * c, ho * wo * co
    with Context(device, w, h, c, radius, max_batch=per, n_slots=2) as ctx:
        if configure:
            configure(ctx)
        for i in range(0, n, per):
            ctx.submit(a.ctypes.data + i * isz, out.ctypes.data + i * osz, min(per, n - i))
        ctx.sync()
    return out


def blur(images, ksize: int = 3, device: int = 0, batch: int = 0):
    """Convenience for Python callers: the reference's blur of a stack of interleaved uint8 images, numpy in -> numpy out.

    images: (H, W), (H, W, C) or (N, H, W, C) uint8.  ksize 3 (the reference kernel, gaussian_kernel.cl:36-41) or
    5.  device: HIP ordinal, or DEVICE_CPU for the host-thread device.  batch: images per submit (0 = all at once, at most 4096).
    Goes through mi_blur_create / mi_blur_submit / mi_blur_sync like any host; there is no other code path behind it.
    A single image comes back as (H, W, C), a 2-D one as (H, W, 1)."""
    a = _images(images, "blur")
    if ksize not in (3, 5):
        raise ValueError("blur: ksize 3 or 5")
    out = _filter_images(a, (ksize - 1) // 2, device, batch)
    return out[0] if a.ndim in (2, 3) else out


def gaussian_blur(images, sigma: float, sigma_y: float | None = None, radius: int = 0, device: int = 0, batch: int = 0):
    """Gaussian blur of any sigma (anisotropic with sigma_y), numpy in -> numpy out, like blur().

    Integer taps from gauss_taps (8 bits per axis), radius 0 = ceil(3 sigma) clamped to [1, 16] per axis.  images: (H, W),
    (H, W, C) or (N, H, W, C) uint8; the result has the same shape.  device: HIP ordinal, or DEVICE_CPU.  Goes through mi_blur_create /
    mi_blur_ctx_set_kernel / mi_blur_submit / mi_blur_sync."""
    a = _images(images, "gaussian_blur")
    kernel = gauss_kernel(sigma, sigma_y, radius)
    return _filter_images(a, 1, device, batch, lambda ctx: ctx.set_kernel(kernel)).reshape(a.shape)


def median_blur(images, ksize: int = 3, device: int = 0, batch: int = 0):
    """Median blur with a ksize x ksize window (ksize odd, 3..15), numpy in -> numpy out, like blur().

    Edges clamp; every output byte is the exact median of its window.  images: (H, W), (H, W, C) or (N, H, W, C) uint8;
    the result has the same shape.  device: HIP ordinal, or DEVICE_CPU.  Goes through mi_blur_create /
    mi_blur_ctx_set_median / mi_blur_submit / mi_blur_sync."""
    if ksize % 2 != 1 or not 3 <= ksize <= 2 * MEDIAN_MAX_RADIUS + 1:
        raise ValueError(f"median_blur: ksize must be odd, 3..{2 * MEDIAN_MAX_RADIUS + 1}")
    a = _images(images, "median_blur")
    return _filter_images(a, 1, device, batch, lambda ctx: ctx.set_median(ksize // 2)).reshape(a.shape)


def _morph(name: str, op: int, images, ksize, device: int, batch: int):
    import operator
    try:
        kx, ky = (ksize, ksize) if not isinstance(ksize, (tuple, list)) else ksize
        kx, ky = operator.index(kx), operator.index(ky)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: ksize is an odd int or a pair (kx, ky) of odd ints") from None
    for k in (kx, ky):
        if k % 2 != 1 or not 1 <= k <= 2 * MORPH_MAX_RADIUS + 1:
            raise ValueError(f"{name}: ksize must be odd, 1..{2 * MORPH_MAX_RADIUS + 1}")
    a = _images(images, name)
    return _filter_images(a, 1, device, batch, lambda ctx: ctx.set_morph(op, kx // 2, ky // 2)).reshape(a.shape)


def erode(images, ksize=3, device: int = 0, batch: int = 0):
    """Greyscale erosion: per channel the minimum of a kx x ky window, numpy in -> numpy out, like blur().

    ksize: an odd int, or a pair (kx, ky) of odd ints (columns, rows), each 1..33.  Edges clamp (pixels outside the image
    are ignored).  images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has the same shape.  device: HIP ordinal,
    or DEVICE_CPU.  Goes through mi_blur_create / mi_blur_ctx_set_morph / mi_blur_submit / mi_blur_sync."""
    return _morph("erode", MORPH_ERODE, images, ksize, device, batch)


def dilate(images, ksize=3, device: int = 0, batch: int = 0):
    """Greyscale dilation: per channel the maximum of a kx x ky window; arguments as erode()."""
    return _morph("dilate", MORPH_DILATE, images, ksize, device, batch)


def morph_gradient(images, ksize=3, device: int = 0, batch: int = 0):
    """Morphological gradient: per channel the window maximum minus the window minimum; arguments as erode()."""
    return _morph("morph_gradient", MORPH_GRADIENT, images, ksize, device, batch)


def bilateral_filter(images, ksize: int = 5, sigma_color: float = 25.0, sigma_space: float = 0.0, device: int = 0, batch: int = 0):
    """Bilateral filter (edge-preserving smoothing) with a ksize x ksize window, numpy in -> numpy out, like blur().

    ksize: odd, 3..17.  sigma_color: the range Gaussian's sigma in grey levels (> 0).  sigma_space: the spatial Gaussian's
    sigma in pixels; <= 0 means ksize / 4.  The tables are integers (Bilateral.gauss), so the result is exact and the same
    on every device.  Each channel is filtered on its own: for colour images this differs from OpenCV's bilateralFilter,
    which measures the range distance in colour space.  images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has
    the same shape.  device: HIP ordinal, or DEVICE_CPU.  Goes through mi_blur_create / mi_blur_ctx_set_bilateral /
    mi_blur_submit / mi_blur_sync."""
    if not isinstance(ksize, int) or isinstance(ksize, bool) or ksize % 2 != 1 or not 3 <= ksize <= 2 * BILATERAL_MAX_RADIUS + 1:
        raise ValueError(f"bilateral_filter: ksize must be odd, 3..{2 * BILATERAL_MAX_RADIUS + 1}")
    if not sigma_color > 0:
        raise ValueError("bilateral_filter: sigma_color must be > 0")
    a = _images(images, "bilateral_filter")
    k = Bilateral.gauss(sigma_space if sigma_space > 0 else ksize / 4.0, sigma_color, ksize // 2)
    return _filter_images(a, 1, device, batch, lambda ctx: ctx.set_bilateral(k)).reshape(a.shape)


def _conv(name: str, images, k: "Conv", device: int, batch: int):
    a = _images(images, name)
    return _filter_images(a, 1, device, batch, lambda ctx: ctx.set_conv(k)).reshape(a.shape)


def filter2d(images, kernel, shift: int = 0, bias: int = 0, mode: str = "sat", kernel2=None, device: int = 0, batch: int = 0):
    """2-D correlation with signed integer taps (OpenCV filter2D's convention: no flip), numpy in -> numpy out, like blur().

    kernel: rows of integer taps, odd sides up to 15 x 15, sum |K| <= 65535.  Per channel acc = sum K * window;
    mode "sat": clamp((acc + bias) >> shift), "abs": clamp((|acc| + bias) >> shift), "mag" (with kernel2, same shape):
    clamp((|acc| + |acc2| + bias) >> shift), each clamped to 0..255; the shift is a floor.  Edges clamp.  images: (H, W),
    (H, W, C) or (N, H, W, C) uint8; the result has the same shape.  device: HIP ordinal, or DEVICE_CPU.  Goes through
    mi_blur_create / mi_blur_ctx_set_conv / mi_blur_submit / mi_blur_sync."""
    import numpy as np
    tab = lambda t: None if t is None else np.asarray(t).tolist()
    k = Conv.from_taps(tab(kernel), shift, bias, mode, tab(kernel2))
    return _conv("filter2d", images, k, device, batch)


def _gradient(name: str, images, axis: str, device: int, batch: int):
    if axis not in ("x", "y", "mag"):
        raise ValueError(f'{name}: axis is "x", "y" or "mag"')
    return _conv(name, images, Conv.preset(f"{name}_{axis}"), device, batch)


def sobel(images, axis: str = "mag", device: int = 0, batch: int = 0):
    """Sobel edge map: axis "x" | "y": min(255, |gradient|) along that axis; "mag": min(255, |gx| + |gy|).  Arguments as filter2d()."""
    return _gradient("sobel", images, axis, device, batch)


def scharr(images, axis: str = "mag", device: int = 0, batch: int = 0):
    """Scharr edge map (taps 3, 10, 3): axis as sobel()."""
    return _gradient("scharr", images, axis, device, batch)


def laplacian(images, connectivity: int = 4, device: int = 0, batch: int = 0):
    """min(255, |Laplacian|) with the 4- or the 8-neighbour 3x3 kernel.  Arguments as filter2d()."""
    if connectivity not in (4, 8):
        raise ValueError("laplacian: connectivity is 4 or 8")
    return _conv("laplacian", images, Conv.preset(f"laplacian{connectivity}"), device, batch)


def sharpen(images, device: int = 0, batch: int = 0):
    """The 3x3 sharpening kernel [0 -1 0; -1 5 -1; 0 -1 0], saturated to 0..255.  Arguments as filter2d()."""
    return _conv("sharpen", images, Conv.preset("sharpen"), device, batch)


def decimated_size(w: int, h: int, sx: int = 2, sy: int = 2, ox: int = 0, oy: int = 0) -> tuple[int, int]:
    """(Wo, Ho) of a w x h image of which column ox + X*sx and row oy + Y*sy are kept (mi_blur_decimated_size)."""
    d = Decimation(int(sx), int(sy), int(ox), int(oy))
    wo, ho = C.c_int(), C.c_int()
    check(lib().mi_blur_decimated_size(int(w), int(h), C.byref(d), C.byref(wo), C.byref(ho)), "mi_blur_decimated_size")
    return wo.value, ho.value


def _down_images(a, kernel: "SepKernel", d: "Decimation", device: int, batch: int):
    """The numpy driver of sep_down, pyr_down and area_down: a (from _images) through _filter_images with
    mi_blur_ctx_set_sep_down; returns the output with the rank of a and the decimated H and W."""
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError("decimating filters: images must not be empty")
    wo, ho = decimated_size(w, h, d.sx, d.sy, d.ox, d.oy)
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_sep_down(kernel, d.sx, d.sy, d.ox, d.oy), (ho, wo))
    return out[0, :, :, 0] if rank == 2 else out[0] if rank == 3 else out


def sep_down(images, kernel: "SepKernel", sx: int = 2, sy: int = 2, ox: int = 0, oy: int = 0, device: int = 0, batch: int = 0):
    """Separable filter and subsampling in one pass, numpy in -> numpy out: the bytes of the separable filter `kernel`
    (as gaussian_blur applies one) at column ox + X*sx and row oy + Y*sy, of which only those are computed.

    Strides 1..4, phases below them.  images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has the same rank with
    the decimated H and W (decimated_size).  device: HIP ordinal, or DEVICE_CPU.  Goes through mi_blur_create /
    mi_blur_ctx_set_sep_down / mi_blur_submit / mi_blur_sync."""
    return _down_images(_images(images, "sep_down"), kernel, Decimation(int(sx), int(sy), int(ox), int(oy)), device, batch)


def _down_preset(name: str, images, preset: int, device: int, batch: int):
    k, d = SepKernel(), Decimation()
    check(lib().mi_blur_sep_down_preset(preset, C.byref(k), C.byref(d)), "mi_blur_sep_down_preset")
    return _down_images(_images(images, name), k, d, device, batch)


def pyr_down(images, device: int = 0, batch: int = 0):
    """One pyramid level: the 5x5 binomial {1,4,6,4,1} and every second pixel, (H, W) -> ((H + 1) // 2, (W + 1) // 2).
    OpenCV's pyrDown taps and sampling grid, but edges clamp and the shift truncates.  Arguments as sep_down()."""
    return _down_preset("pyr_down", images, DOWN_PYR, device, batch)


def area_down(images, factor: int = 2, device: int = 0, batch: int = 0):
    """Area downscale by 2 or 4: the truncated mean of each factor x factor block (edge blocks clamp).  Arguments as sep_down()."""
    if factor not in (2, 4):
        raise ValueError("area_down: factor is 2 or 4")
    return _down_preset("area_down", images, DOWN_AREA2 if factor == 2 else DOWN_AREA4, device, batch)


def resize_coord(n_in: int, n_out: int, X: int, mode="bilinear") -> tuple[int, int, int]:
    """(a, b, f) of one axis of the resize for output index X of n_out over n_in input samples (mi_blur_resize_coord):
    input samples a <= b <= a + 1 and the weight f of b in 0..2048; nearest gives (i, i, 0)."""
    a, b, f = C.c_int(), C.c_int(), C.c_int()
    check(lib().mi_blur_resize_coord(int(n_in), int(n_out), _resize_mode(mode), int(X), C.byref(a), C.byref(b), C.byref(f)),
          "mi_blur_resize_coord")
    return a.value, b.value, f.value


def resize(images, size, mode="bilinear", device: int = 0, batch: int = 0):
    """Resize to size = (out_width, out_height), numpy in -> numpy out: exact fixed-point bilinear (11 fraction bits, one
    final rounding) or nearest, pixel centres aligned, any ratio (include/mi_blur.h has the definition).

    images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has the same rank with out_height and out_width.
    device: HIP ordinal, or DEVICE_CPU.  A reduction by more than 2x aliases: area_down / pyr_down first.  Goes through
    mi_blur_create / mi_blur_ctx_set_resize / mi_blur_submit / mi_blur_sync."""
    a = _images(images, "resize")
    wo, ho = int(size[0]), int(size[1])
    m = _resize_mode(mode)
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError("resize: images must not be empty")
    if wo < 1 or ho < 1:
        raise ValueError("resize: size is (out_width, out_height), both at least 1")
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_resize(wo, ho, m), (ho, wo))
    return out[0, :, :, 0] if rank == 2 else out[0] if rank == 3 else out


def area_coord(n_in: int, n_out: int, X: int) -> tuple[int, int, int, int]:
    """(i_lo, i_hi, w_lo, w_hi) of one axis of the area resize for output index X of n_out over n_in input samples
    (mi_blur_area_coord): the first and the last tap and their weights; w_hi = 0 when there is one tap (w_lo = n_in then);
    every tap between them weighs n_out."""
    i_lo, i_hi, w_lo, w_hi = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().mi_blur_area_coord(int(n_in), int(n_out), int(X), C.byref(i_lo), C.byref(i_hi), C.byref(w_lo), C.byref(w_hi)),
          "mi_blur_area_coord")
    return i_lo.value, i_hi.value, w_lo.value, w_hi.value


def area_resize(images, size, device: int = 0, batch: int = 0):
    """Area resize to size = (out_width, out_height), numpy in -> numpy out: every output pixel is the exact box average
    of the input area under it, rounded once, half up (include/mi_blur.h has the definition): the anti-aliased reduction
    at any ratio up to AREA_MAX_RATIO per axis.  Enlarging is valid and replicates pixels at integer ratios.

    images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has the same rank with out_height and out_width.
    device: HIP ordinal, or DEVICE_CPU.  Goes through mi_blur_create / mi_blur_ctx_set_area / mi_blur_submit / mi_blur_sync."""
    a = _images(images, "area_resize")
    wo, ho = int(size[0]), int(size[1])
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError("area_resize: images must not be empty")
    if wo < 1 or ho < 1:
        raise ValueError("area_resize: size is (out_width, out_height), both at least 1")
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_area(wo, ho), (ho, wo))
    return out[0, :, :, 0] if rank == 2 else out[0] if rank == 3 else out


def color_preset(name) -> "Color":
    """The preset `name` (a key of COLOR_CODES, or its id) as a Color (mi_blur_color_preset)."""
    k = Color()
    code = COLOR_CODES.get(name.lower()) if isinstance(name, str) else int(name)
    if code is None:
        raise ValueError(f"color_preset: one of {sorted(COLOR_CODES)}")
    check(lib().mi_blur_color_preset(code, C.byref(k)), "mi_blur_color_preset")
    return k


def _color_set_lut(k: "Color", lut, name: str) -> None:
    """lut (256 entries for every channel, or out_channels x 256) into k, lut_on = 1."""
    import numpy as np
    t = np.asarray(lut)
    if t.shape == (256,):
        t = np.broadcast_to(t, (k.out_channels, 256))
    if t.shape != (k.out_channels, 256) or t.min() < 0 or t.max() > 255:
        raise ValueError(f"{name}: lut is 256 entries, or out_channels x 256, each 0..255")
    t = np.ascontiguousarray(t, dtype=np.uint8)
    for o in range(k.out_channels):
        C.memmove(k.lut[o], t[o].ctypes.data, 256)
    k.lut_on = 1


def _color_run(images, make, device: int, batch: int, name: str):
    """images through the Color that make(channels) returns: (H, W), (H, W, C) or (N, H, W, C) in; (N, H, W, Co) out of a
    stack, (H, W, Co) out of a single image, and (H, W) where that has one channel."""
    a, rank = _tone_stack(images, name)
    k = make(a.shape[3])
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_color(k), None, k.out_channels)
    if rank == 4:
        return out
    return out[0, :, :, 0] if k.out_channels == 1 else out[0]


def color_transform(images, matrix, bias=None, shift: int = 0, lut=None, device: int = 0, batch: int = 0):
    """The colour transform, numpy in -> numpy out (include/mi_blur.h has the definition): per pixel and output channel o
    clamp((bias[o] + sum_i matrix[o][i] * in[i]) >> shift, 0, 255), then through lut when one is given.

    matrix: Co x C integers (Co 1..4, C the images' channels); bias: Co integers (default 0); shift 0..16; lut: 256 entries
    for every channel, or Co x 256.  images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has Co channels (a
    one-channel result of a 2-D or 3-D input comes back as (H, W)).  device: HIP ordinal, or DEVICE_CPU.
    Goes through mi_blur_create / mi_blur_ctx_set_color / mi_blur_submit / mi_blur_sync."""
    import numpy as np
    m = np.asarray(matrix, dtype=np.int64)
    if m.ndim != 2 or not 1 <= m.shape[0] <= COLOR_MAX_CHANNELS:
        raise ValueError("color_transform: matrix is Co x C integers, Co 1..4")
    b = np.zeros(m.shape[0], np.int64) if bias is None else np.asarray(bias, dtype=np.int64)
    if b.shape != (m.shape[0],) or np.abs(m).max(initial=0) >= 2**31 or np.abs(b).max(initial=0) >= 2**31:
        raise ValueError("color_transform: bias is Co integers; every entry within 32 bits")

    def make(c):
        if m.shape[1] != c:
            raise ValueError(f"color_transform: matrix has {m.shape[1]} columns, the images {c} channels")
        k = Color()
        k.out_channels, k.shift = m.shape[0], int(shift)
        for o in range(m.shape[0]):
            for i in range(c):
                k.m[o][i] = int(m[o, i])
            k.bias[o] = int(b[o])
        if lut is not None:
            _color_set_lut(k, lut, "color_transform")
        return k
    return _color_run(images, make, device, batch, "color_transform")


def cvt_color(images, code: str, device: int = 0, batch: int = 0):
    """Colour conversion by preset, numpy in -> numpy out: code is one of COLOR_CODES ("rgb2gray", "bgr2gray", "gray2rgb",
    "rgb2bgr", "rgba2bgra", "rgba2rgb", "rgb2rgba", "rgb2ycbcr", "ycbcr2rgb"; include/mi_blur.h has the table).  A 2-D
    array is one grey image; a one-channel result of a 3-D input comes back as (H, W).  Not OpenCV's cvtColor bit for bit."""
    k = color_preset(code)
    return _color_run(images, lambda c: k, device, batch, "cvt_color")


def apply_lut(images, lut, device: int = 0, batch: int = 0):
    """Every byte through a table (OpenCV's LUT): lut is 256 entries for every channel, or C x 256."""
    def make(c):
        k = Color()
        check(lib().mi_blur_color_identity(c, C.byref(k)), "mi_blur_color_identity")
        _color_set_lut(k, lut, "apply_lut")
        return k
    return _color_run(images, make, device, batch, "apply_lut")


def gamma_correct(images, gamma: float, device: int = 0, batch: int = 0):
    """out = round(255 * (in / 255) ** gamma), through the table of mi_blur_color_lut_gamma."""
    t = (C.c_uint8 * 256)()
    check(lib().mi_blur_color_lut_gamma(float(gamma), t), "mi_blur_color_lut_gamma")
    return apply_lut(images, list(t), device, batch)


def threshold(images, t: int, lo: int = 0, hi: int = 255, device: int = 0, batch: int = 0):
    """out = hi where in > t, else lo (OpenCV's THRESH_BINARY with two levels), through the table of
    mi_blur_color_lut_threshold."""
    tab = (C.c_uint8 * 256)()
    check(lib().mi_blur_color_lut_threshold(int(t), int(lo), int(hi), tab), "mi_blur_color_lut_threshold")
    return apply_lut(images, list(tab), device, batch)


def _tone_stack(images, name: str):
    """(images as (N, H, W, C), the rank they came with) for the colour transform and the families outside Filter:
    non-empty images of 1..4 channels."""
    a = _images(images, name)
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError(f"{name}: images must not be empty")
    if c > COLOR_MAX_CHANNELS:
        raise ValueError(f"{name}: at most {COLOR_MAX_CHANNELS} channels")
    return a, rank


def _batches(n: int, batch: int):
    """(first image, images) of every call on n images, `batch` images per call (0 = all at once)."""
    per = batch if batch > 0 else max(n, 1)
    for i in range(0, n, per):
        yield i, min(per, n - i)


def _unstack(out, rank: int, pixels: bool = True):
    """out, one entry per image, in the rank the images came with (_tone_stack): a stack's, or one image's; of one grey
    image (H, W) without the channel axis too where out is pixels (N, H, W, C) and not tables."""
    return out if rank == 4 else out[0, :, :, 0] if pixels and rank == 2 else out[0]


def _channel_mask(channels, c: int, name: str) -> int:
    """The mask of the channel indices `channels` of c channels; None (all) is 0."""
    mask = 0
    for ch in (() if channels is None else channels):
        if not 0 <= int(ch) < c:
            raise ValueError(f"{name}: channel {ch} of {c}")
        mask |= 1 << int(ch)
    return mask


def _tone(mode, clip_q16, joint, channels, c: int, name: str) -> "Tone":
    """A Tone for images of c channels.  mode: a key of TONE_MODES; clip_q16: (lo, hi) Q16 integers; channels: None (all)
    or the indices of the channels to transform."""
    if mode not in TONE_MODES:
        raise ValueError(f"{name}: mode is one of {sorted(TONE_MODES)}")
    lo, hi = (int(v) for v in clip_q16)
    return Tone(TONE_MODES[mode], lo, hi, int(bool(joint)), _channel_mask(channels, c, name))


def _clip_q16(clip, name: str) -> tuple[int, int]:
    """A fraction of the pixels, or a (lo, hi) pair of fractions, each in [0, 0.5), as Q16 integers (floor)."""
    import math
    pair = tuple(clip) if isinstance(clip, (tuple, list)) else (clip, clip)
    if len(pair) != 2 or not all(0.0 <= float(v) < 0.5 for v in pair):
        raise ValueError(f"{name}: clip is a fraction in [0, 0.5), or a (lo, hi) pair of them")
    return tuple(int(math.floor(float(v) * 65536.0)) for v in pair)


def _tone_run(a, tone: "Tone", device: int, batch: int, name: str):
    """a (N, H, W, C) through mi_blur_run_tone, `batch` images per call (0 = all at once)."""
    import numpy as np
    n, h, w, c = a.shape
    out = np.empty_like(a)
    for i, k in _batches(n, batch):
        check(lib().mi_blur_run_tone(device, a[i:].ctypes.data, out[i:].ctypes.data, None, w, h, c, k, C.byref(tone)), name)
    return out


def histogram(images, device: int = 0, batch: int = 0):
    """The histogram of every image and channel (mi_blur_run_hist): uint32 of shape (N, C, 256) for a stack (N, H, W, C),
    (C, 256) for one image (H, W, C) or (H, W).  Exact counts.  device: HIP ordinal, or DEVICE_CPU; batch: images per
    call (0 = all at once)."""
    import numpy as np
    a, rank = _tone_stack(images, "histogram")
    n, h, w, c = a.shape
    out = np.empty((n, c, HIST_BINS), np.uint32)
    for i, k in _batches(n, batch):
        check(lib().mi_blur_run_hist(device, a[i:].ctypes.data, out[i:].ctypes.data, w, h, c, k), "mi_blur_run_hist")
    return _unstack(out, rank, False)


def tone_tables(hist, mode: str = "equalize", clip=(0, 0), joint: bool = False, channels=None):
    """The tone tables of histograms (mi_blur_tone_tables; include/mi_blur.h has the definition): hist uint32 (C, 256) or
    (N, C, 256) -> uint8 of the same shape.  mode: "equalize" | "stretch"; clip: the (lo, hi) shares of the pixels clipped
    by "stretch", Q16 INTEGERS 0..32767 as the ABI takes them; joint: one table from the summed histograms; channels:
    the indices of the channels to transform (None = all), the others get the identity."""
    import numpy as np
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.ndim not in (2, 3) or h.shape[-1] != HIST_BINS or not 1 <= h.shape[-2] <= COLOR_MAX_CHANNELS:
        raise ValueError("tone_tables: hist is uint32 of shape (C, 256) or (N, C, 256), C 1..4")
    c = h.shape[-2]
    t = _tone(mode, clip, joint, channels, c, "tone_tables")
    out = np.empty(h.shape, np.uint8)
    hs, os_ = h.reshape(-1, c, HIST_BINS), out.reshape(-1, c, HIST_BINS)
    for i in range(hs.shape[0]):
        check(lib().mi_blur_tone_tables(hs[i].ctypes.data, c, C.byref(t), os_[i].ctypes.data), "mi_blur_tone_tables")
    return out


def equalize_hist(images, mode: str = "channel", device: int = 0, batch: int = 0):
    """Histogram equalisation with one table per image (mi_blur_run_tone, MI_BLUR_TONE_EQUALIZE), numpy in -> numpy out of
    the same shape.  mode "channel": every channel by its own histogram; "joint": one table per image from the sum of
    its channels' histograms; "luma" (3 channels): cvt_color(rgb2ycbcr), Y equalised, cvt_color(ycbcr2rgb).  OpenCV's
    equalizeHist formula as an exact ratio, not its bytes."""
    if mode not in ("channel", "joint", "luma"):
        raise ValueError('equalize_hist: mode is "channel", "joint" or "luma"')
    a, rank = _tone_stack(images, "equalize_hist")
    c = a.shape[3]
    if mode == "luma":
        if c != 3:
            raise ValueError('equalize_hist: "luma" needs 3 channels')
        ycc = cvt_color(a, "rgb2ycbcr", device, batch)
        out = cvt_color(_tone_run(ycc, _tone("equalize", (0, 0), False, (0,), 3, "equalize_hist"), device, batch, "equalize_hist"),
                        "ycbcr2rgb", device, batch)
    else:
        out = _tone_run(a, _tone("equalize", (0, 0), mode == "joint", None, c, "equalize_hist"), device, batch, "equalize_hist")
    return _unstack(out, rank)


def auto_levels(images, clip=0.0, joint: bool = True, channels=None, device: int = 0, batch: int = 0):
    """Contrast stretch with one table per image (mi_blur_run_tone, MI_BLUR_TONE_STRETCH): the darkest `clip` share of
    the pixels goes to 0, the brightest to 255, linear between them; clip = 0 is min-max normalisation.  clip: a
    fraction in [0, 0.5) or a (lo, hi) pair, converted to Q16 with floor.  joint (default): one table per image from
    all transformed channels, which keeps the colour balance; channels: indices to transform (None = all)."""
    a, rank = _tone_stack(images, "auto_levels")
    t = _tone("stretch", _clip_q16(clip, "auto_levels"), joint, channels, a.shape[3], "auto_levels")
    out = _tone_run(a, t, device, batch, "auto_levels")
    return _unstack(out, rank)


def _clahe(clip_limit, tiles, channels, c: int, name: str) -> "Clahe":
    """A Clahe for images of c channels.  clip_limit: OpenCV's clipLimit, 0..256 (0 = no clipping), taken as
    floor(clip_limit * 256); tiles: (tiles_x, tiles_y); channels: None (all) or the indices of the channels to transform."""
    import math
    if not 0.0 <= float(clip_limit) <= 256.0:
        raise ValueError(f"{name}: clip_limit is in 0..256")
    tx, ty = (int(v) for v in tiles)
    return Clahe(tx, ty, int(math.floor(float(clip_limit) * 256.0)), _channel_mask(channels, c, name))


def _clahe_run(a, k: "Clahe", device: int, batch: int, name: str, want_work: bool = False):
    """a (N, H, W, C) through mi_blur_run_clahe, `batch` images per call (0 = all at once): the output, and with want_work
    the tile histograms uint32 (N, TY, TX, C, 256) and the tile tables uint8 of the same shape."""
    import numpy as np
    n, h, w, c = a.shape
    out = np.empty_like(a)
    shape = (n, k.tiles_y, k.tiles_x, c, HIST_BINS)
    hist, tables = (np.empty(shape, np.uint32), np.empty(shape, np.uint8)) if want_work else (None, None)
    for i, m in _batches(n, batch):
        words = m * k.tiles_y * k.tiles_x * c * HIST_BINS
        work = np.empty(5 * words, np.uint8) if want_work else None
        check(lib().mi_blur_run_clahe(device, a[i:].ctypes.data, out[i:].ctypes.data, None if work is None else work.ctypes.data,
                                      w, h, c, m, C.byref(k)), name)
        if want_work:
            hist[i:i + m] = work[:4 * words].view(np.uint32).reshape((m,) + shape[1:])
            tables[i:i + m] = work[4 * words:].reshape((m,) + shape[1:])
    return (out, hist, tables) if want_work else out


def clahe(images, clip_limit: float = 2.0, tiles=(8, 8), mode: str = "channel", channels=None, device: int = 0, batch: int = 0):
    """CLAHE (mi_blur_run_clahe; include/mi_blur.h, "CLAHE" has the definition), numpy in -> numpy out of the same shape:
    every tile of a tiles = (tiles_x, tiles_y) grid gets its own table from its histogram clipped at clip_limit (OpenCV's
    clipLimit; 0 = no clipping), and every pixel the blend of the four tables around it.  mode "channel": every channel
    (or those of `channels`) on its own; "luma" (3 channels): cvt_color(rgb2ycbcr), CLAHE on Y, cvt_color(ycbcr2rgb).
    The tiles are the image's own (no padding) and the arithmetic is integer: OpenCV's formula, not its bytes."""
    if mode not in ("channel", "luma"):
        raise ValueError('clahe: mode is "channel" or "luma"')
    a, rank = _tone_stack(images, "clahe")
    c = a.shape[3]
    if mode == "luma":
        if c != 3:
            raise ValueError('clahe: "luma" needs 3 channels')
        ycc = cvt_color(a, "rgb2ycbcr", device, batch)
        out = cvt_color(_clahe_run(ycc, _clahe(clip_limit, tiles, (0,), 3, "clahe"), device, batch, "clahe"), "ycbcr2rgb", device, batch)
    else:
        out = _clahe_run(a, _clahe(clip_limit, tiles, channels, c, "clahe"), device, batch, "clahe")
    return _unstack(out, rank)


def clahe_tables(images, clip_limit: float = 2.0, tiles=(8, 8), channels=None, device: int = 0, batch: int = 0):
    """(hist, tables) of clahe(): the raw tile histograms uint32 (N, TY, TX, C, 256) and the tile tables uint8 of the same
    shape (without the leading N for one image)."""
    a, rank = _tone_stack(images, "clahe_tables")
    _, hist, tables = _clahe_run(a, _clahe(clip_limit, tiles, channels, a.shape[3], "clahe_tables"), device, batch, "clahe_tables", True)
    return _unstack(hist, rank, False), _unstack(tables, rank, False)


def clahe_coord(size: int, tiles: int, x: int) -> tuple[int, int, int]:
    """(t0, t1, frac) of pixel x on an axis of `size` pixels and `tiles` tiles (mi_blur_clahe_coord)."""
    t0, t1, f = C.c_int(), C.c_int(), C.c_int()
    check(lib().mi_blur_clahe_coord(int(size), int(tiles), int(x), C.byref(t0), C.byref(t1), C.byref(f)), "mi_blur_clahe_coord")
    return t0.value, t1.value, f.value


def integral(images, square: bool = False, pad: bool = False, device: int = 0, batch: int = 0):
    """The integral image of every image and channel (mi_blur_run_integral; include/mi_blur.h, "Integral images, and box
    filters", has the definition): uint32 of the images' own shape, entry (y, x) = the sum over rows <= y and columns <= x,
    modulo 2^32.  square=True: of the squares instead.  pad=True: OpenCV's layout, one row and one column of zeros in
    front, (H + 1) x (W + 1), padded on the host.  device: HIP ordinal, or DEVICE_CPU; batch: images per call (0 = all)."""
    import numpy as np
    a, rank = _tone_stack(images, "integral")
    n, h, w, c = a.shape
    out = np.empty((n, h, w, c), np.uint32)
    for i, k in _batches(n, batch):
        t = out[i:].ctypes.data
        check(lib().mi_blur_run_integral(device, a[i:].ctypes.data, None if square else t, t if square else None, w, h, c, k), "mi_blur_run_integral")
    if pad:
        out = np.pad(out, ((0, 0), (1, 0), (1, 0), (0, 0)))
    return _unstack(out, rank)


def rect_sum(table, x0: int, y0: int, x1: int, y1: int):
    """The sum over columns x0..x1 and rows y0..y1 (inclusive) from a table of integral() (pad=False), modulo 2^32: exact
    whenever the true sum is below 2^32.  table: (..., H, W) for grey images or (..., H, W, C); numpy only."""
    import numpy as np
    t = np.asarray(table)
    if t.dtype != np.uint32 or t.ndim < 2:
        raise ValueError("rect_sum: table is a uint32 array from integral()")
    grey = t.ndim == 2
    if grey:
        t = t[:, :, None]
    h, w = t.shape[-3], t.shape[-2]
    if not (0 <= x0 <= x1 < w and 0 <= y0 <= y1 < h):
        raise ValueError("rect_sum: 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H")
    at = lambda y, x: t[..., y, x, :] if x >= 0 and y >= 0 else np.zeros(t.shape[:-3] + t.shape[-1:], np.uint32)
    s = at(y1, x1) - at(y0 - 1, x1) - at(y1, x0 - 1) + at(y0 - 1, x0 - 1)          # uint32: wraps, as the definition says
    return s[..., 0] if grey else s


def _box(ksize, op: int, offset: int, invert: bool, name: str) -> "Box":
    pair = tuple(ksize) if isinstance(ksize, (tuple, list)) else (ksize, ksize)
    kx, ky = pair if len(pair) == 2 else (0, 0)
    for k in (kx, ky):
        if not isinstance(k, int) or k < 1 or k % 2 == 0 or k > 2 * BOX_MAX_RADIUS + 1:
            raise ValueError(f"{name}: ksize is an odd integer 1..{2 * BOX_MAX_RADIUS + 1}, or a pair (kx, ky) of them")
    if not -255 <= int(offset) <= 255:
        raise ValueError(f"{name}: offset is -255..255")
    return Box(op, kx // 2, ky // 2, int(offset), int(bool(invert)))


def _box_run(images, k: "Box", device: int, batch: int, name: str):
    import numpy as np
    a, rank = _tone_stack(images, name)
    n, h, w, c = a.shape
    out = np.empty_like(a)
    for i, m in _batches(n, batch):
        check(lib().mi_blur_run_box(device, a[i:].ctypes.data, out[i:].ctypes.data, w, h, c, m, C.byref(k)), "mi_blur_run_box")
    return _unstack(out, rank)


def box_blur(images, ksize, device: int = 0, batch: int = 0):
    """The box mean over a kx x ky window (mi_blur_run_box, BOX_MEAN), clamp-to-edge, rounded once, half up; numpy in ->
    numpy out of the same shape.  ksize: an odd int or (kx, ky), each at most 255.  The cost does not depend on the window."""
    return _box_run(images, _box(ksize, BOX_MEAN, 0, False, "box_blur"), device, batch, "box_blur")


def local_stddev(images, ksize, device: int = 0, batch: int = 0):
    """The standard deviation over a kx x ky window (BOX_STDDEV), clamp-to-edge, rounded once, half up: 0..128."""
    return _box_run(images, _box(ksize, BOX_STDDEV, 0, False, "local_stddev"), device, batch, "local_stddev")


def adaptive_threshold(images, ksize, offset: int = 0, invert: bool = False, device: int = 0, batch: int = 0):
    """The adaptive threshold (BOX_THRESHOLD): 255 where a pixel exceeds the mean of its kx x ky window minus `offset`
    (the mean not rounded), else 0; invert swaps the two.  OpenCV's adaptiveThreshold with ADAPTIVE_THRESH_MEAN_C and
    C = offset, but not its bytes, which round the mean first."""
    return _box_run(images, _box(ksize, BOX_THRESHOLD, offset, invert, "adaptive_threshold"), device, batch, "adaptive_threshold")


def _dist(metric, sites, limit: int, byte_op: int, invert: bool, name: str) -> "Dist":
    code = DIST_METRICS.get(metric.lower()) if isinstance(metric, str) else None
    if code is None:
        raise ValueError(f"{name}: metric is one of {sorted(DIST_METRICS)}")
    if sites not in ("zero", "nonzero"):
        raise ValueError(f'{name}: sites is "zero" or "nonzero"')
    if not isinstance(limit, int) or not 0 <= limit <= DIST_MAX_LIMIT:
        raise ValueError(f"{name}: a limit or radius is an integer 0..{DIST_MAX_LIMIT}")
    return Dist(code, int(sites == "nonzero"), limit, byte_op, int(bool(invert)))


def _dist_run(images, k: "Dist", table: bool, device: int, batch: int, name: str):
    import numpy as np
    a, rank = _tone_stack(images, name)
    n, h, w, c = a.shape
    out = np.empty(a.shape, np.uint32 if table else np.uint8)
    run, export = (lib().mi_blur_run_dist, "mi_blur_run_dist") if table else (lib().mi_blur_run_dist_u8, "mi_blur_run_dist_u8")
    for i, m in _batches(n, batch):
        check(run(device, a[i:].ctypes.data, out[i:].ctypes.data, w, h, c, m, C.byref(k)), export)
    return _unstack(out, rank)


def distance_transform(images, metric: str = "l2", sites: str = "zero", limit: int = 0, device: int = 0, batch: int = 0):
    """The exact distance of every pixel to the nearest site of its image and channel (mi_blur_run_dist; include/mi_blur.h,
    "Exact distance transform", has the definition): uint32 of the images' shape.  metric "l2": the SQUARED Euclidean
    distance; "l1": city block; "linf": chessboard.  sites "zero" (OpenCV's distanceTransform): the zero pixels are the
    sites; "nonzero": the others.  A channel without a site, and with a limit every pixel farther than `limit` from one,
    holds DIST_NONE.  device: HIP ordinal, or DEVICE_CPU; batch: images per call (0 = all)."""
    return _dist_run(images, _dist(metric, sites, limit, DIST_BYTE, False, "distance_transform"), True, device, batch, "distance_transform")


def distance_transform_u8(images, metric: str = "l2", sites: str = "zero", limit: int = 0, device: int = 0, batch: int = 0):
    """The same as bytes (mi_blur_run_dist_u8, DIST_BYTE): the distance itself, saturated at 255; for "l2" the square root
    rounded once, half up.  255 where distance_transform() holds DIST_NONE."""
    return _dist_run(images, _dist(metric, sites, limit, DIST_BYTE, False, "distance_transform_u8"), False, device, batch, "distance_transform_u8")


def _disc(images, radius: int, metric, sites: str, invert: bool, device: int, batch: int, name: str):
    if radius == 0:
        raise ValueError(f"{name}: radius is an integer 1..{DIST_MAX_LIMIT}")
    return _dist_run(images, _dist(metric, sites, radius, DIST_WITHIN, invert, name), False, device, batch, name)


def disc_dilate(images, radius: int, metric: str = "l2", device: int = 0, batch: int = 0):
    """Dilation of MASKS (zero / non-zero pixels) by the metric's ball of `radius` (1..32767): a disc ("l2"), a diamond
    ("l1") or a (2 radius + 1)-square ("linf").  255 where a non-zero pixel lies within `radius`, else 0
    (mi_blur_run_dist_u8, DIST_WITHIN).  The cost does not grow with the area of the element.  Opening is disc_erode then
    disc_dilate, closing disc_dilate then disc_erode: two calls."""
    return _disc(images, radius, metric, "nonzero", False, device, batch, "disc_dilate")


def disc_erode(images, radius: int, metric: str = "l2", device: int = 0, batch: int = 0):
    """Erosion of MASKS (zero / non-zero pixels) by the same element: 255 where no zero pixel lies within `radius`, else 0.
    Pixels outside the image do not count as zero.  Opening and closing are two calls: see disc_dilate."""
    return _disc(images, radius, metric, "zero", True, device, batch, "disc_erode")


def dist_value(k: "Dist", t: int) -> int:
    """The byte of the byte struct k for the table value t (mi_blur_dist_value); -1 for an invalid k or a t no image gives."""
    return lib().mi_blur_dist_value(C.byref(k), int(t))


def _match_method(method, name: str) -> int:
    code = MATCH_METHODS.get(method.lower()) if isinstance(method, str) else None
    if code is None:
        raise ValueError(f"{name}: method is one of {sorted(MATCH_METHODS)}")
    return code


def match_template(images, template, method: str = "zncc", device: int = 0, batch: int = 0):
    """Every position's match of `template` in its image (mi_blur_run_match; include/mi_blur.h, "Template matching and
    peak search", has the definition): (N, Ho, Wo) or (Ho, Wo), Ho = H - th + 1, Wo = W - tw + 1, the channels summed.
    method "sqdiff" | "ccorr" | "sad": the exact sums, uint32; "ncc" | "zncc": int32 scores, MATCH_ONE = 1.0.  images:
    (H, W), (H, W, C) or (N, H, W, C) uint8.  template: (th, tw[, C]), one for every image, or (N, th, tw[, C]), one per
    image; th, tw <= 255 and th * tw * C <= 65536.  device: HIP ordinal, or DEVICE_CPU; batch: images per call (0 = all)."""
    import numpy as np
    code = _match_method(method, "match_template")
    a, rank = _tone_stack(images, "match_template")
    n, h, w, c = a.shape
    t = np.ascontiguousarray(template)
    if t.dtype != np.uint8:
        raise ValueError("match_template: the template is uint8")
    if c == 1 and (t.ndim == 2 or (rank == 2 and t.ndim == 3)):
        t = t[..., None]                                                # grey images given without the channel axis: so is the template
    if t.ndim == 3:
        shared = True
    elif t.ndim == 4:
        shared = False
    else:
        raise ValueError("match_template: the template is (th, tw[, C]) or (N, th, tw[, C])")
    if t.shape[-1] != c or (not shared and t.shape[0] != n):
        raise ValueError("match_template: the template has the images' channels and, per image, their number")
    th, tw = t.shape[-3], t.shape[-2]
    if not (1 <= tw <= min(w, MATCH_MAX_SIDE) and 1 <= th <= min(h, MATCH_MAX_SIDE) and tw * th * c <= MATCH_MAX_AREA):
        raise ValueError(f"match_template: a template is 1..{MATCH_MAX_SIDE} a side, inside the image, and th * tw * C <= {MATCH_MAX_AREA}")
    k = Match(code, tw, th, int(shared))
    out = np.empty((n, h - th + 1, w - tw + 1), np.int32 if code >= MATCH_NCC else np.uint32)
    for i, m in _batches(n, batch):
        check(lib().mi_blur_run_match(device, a[i:].ctypes.data, (t if shared else t[i:]).ctypes.data, out[i:].ctypes.data, w, h, c, m, C.byref(k)),
              "mi_blur_run_match")
    return out if rank == 4 else out[0]


def match_peak(table, device: int = 0):
    """minMaxLoc of a match table (mi_blur_run_match_peak): per image (min, (x, y), max, (x, y)), ties to the first entry in
    row-major order.  table: (Ho, Wo) or (N, Ho, Wo), uint32 or int32; one tuple, or a list of N."""
    import numpy as np
    t = np.ascontiguousarray(table)
    if t.dtype not in (np.uint32, np.int32) or t.ndim not in (2, 3) or t.size == 0:
        raise ValueError("match_peak: a non-empty uint32 or int32 table, (Ho, Wo) or (N, Ho, Wo)")
    stack = t if t.ndim == 3 else t[None]
    n, ho, wo = stack.shape
    peaks = np.empty((n, 6), np.int64)
    check(lib().mi_blur_run_match_peak(device, stack.ctypes.data, int(t.dtype == np.int32), wo, ho, n, peaks.ctypes.data), "mi_blur_run_match_peak")
    res = [(int(p[0]), (int(p[1]), int(p[2])), int(p[3]), (int(p[4]), int(p[5]))) for p in peaks]
    return res if t.ndim == 3 else res[0]


def find_template(images, template, method: str = "zncc", device: int = 0):
    """The best position of the template in every image and its value: ((x, y), value), the maximum for "ccorr", "ncc" and
    "zncc", the minimum for "sqdiff" and "sad"; one pair, or a list of N."""
    table = match_template(images, template, method, device)
    peaks = match_peak(table, device)
    least = _match_method(method, "find_template") in (MATCH_SQDIFF, MATCH_SAD)
    pick = lambda p: (p[1], p[0]) if least else (p[3], p[2])
    return [pick(p) for p in peaks] if isinstance(peaks, list) else pick(peaks)


def match_value(method, A: int, sum_at: int, sum_a: int, sum_aa: int, sum_t: int, sum_tt: int):
    """The score of the sums (mi_blur_match_value), method "ncc" | "zncc" or its code; None for anything the export refuses,
    sums beyond 32 bits included."""
    code = MATCH_METHODS.get(method.lower(), -1) if isinstance(method, str) else int(method)
    args = (A, sum_at, sum_a, sum_aa, sum_t, sum_tt)
    if any(not 0 <= int(v) < 1 << 32 for v in args):
        return None
    v = lib().mi_blur_match_value(code, *(int(v) for v in args))
    return None if v == -(1 << 31) else v


def arith_preset(name) -> "Arith":
    """The preset `name` (a key of ARITH_PRESETS, or its id) as an Arith (mi_blur_arith_preset), plane and shared flags 0."""
    k = Arith()
    code = ARITH_PRESETS.get(name.lower()) if isinstance(name, str) else int(name)
    if code is None:
        raise ValueError(f"arith_preset: one of {sorted(ARITH_PRESETS)}")
    check(lib().mi_blur_arith_preset(code, C.byref(k)), "mi_blur_arith_preset")
    return k


def arith_value(k: "Arith", a: int, b: int, m: int = 0) -> int:
    """The output byte of k for the operand bytes a, b and (LERP) m: mi_blur_arith_value, the definition for one byte.
    -1 for an invalid k or an operand outside 0..255."""
    return lib().mi_blur_arith_value(C.byref(k), int(a), int(b), int(m))


def _arith_operand(x, shape, name: str, what: str):
    """(x as a contiguous uint8 array, plane, shared) for an operand of images of the stack shape (N, H, W, C):
    (N, H, W, C) full; (H, W, C) one image for all; (N, H, W, 1) a plane; (H, W, 1) or (H, W) one plane for all.  A
    one-channel or single image makes "plane" or "shared" another name of the same bytes."""
    n, h, w, c = shape
    x = _images(x, name)
    if x.ndim == 4 and x.shape in ((n, h, w, c), (n, h, w, 1)):
        return x, int(x.shape[3] != c), 0
    if x.ndim == 3 and x.shape in ((h, w, c), (h, w, 1)):
        return x, int(x.shape[2] != c), 1
    if x.ndim == 2 and x.shape == (h, w):
        return x, int(c != 1), 1
    raise ValueError(f"{name}: {what} of shape {x.shape} does not go with images of shape {shape}: (N, H, W, C), (H, W, C), "
                     "(N, H, W, 1), (H, W, 1) or (H, W)")


def arith(a, b, k: "Arith", mask=None, device: int = 0, batch: int = 0):
    """Two-image arithmetic (mi_blur_run_arith; include/mi_blur.h, "Two-image arithmetic", has the definition): every
    byte of `a` combined with the byte of `b` (and, for ARITH_LERP, of `mask`) by k's operation, numpy in -> numpy out
    of a's shape.  a: (N, H, W, C), (H, W, C) or (H, W) uint8.  b and mask, against a's stack shape (N, H, W, C):
    (N, H, W, C) full; (H, W, C) one image shared by the batch; (N, H, W, 1) one plane per image, applied to every
    channel; (H, W, 1) or (H, W) one shared plane.  k's plane and shared flags are set from these shapes.  mask is
    required for ARITH_LERP and refused otherwise.  device: HIP ordinal, or DEVICE_CPU; batch: images per call (0 = all
    at once), which cuts all unshared operands alike."""
    import numpy as np
    a, rank = _tone_stack(a, "arith")
    n, h, w, c = a.shape
    q = Arith.from_buffer_copy(k)
    if (q.op == ARITH_LERP) != (mask is not None):
        raise ValueError("arith: a mask goes with ARITH_LERP and with nothing else")
    b, q.b_plane, q.b_shared = _arith_operand(b, a.shape, "arith", "b")
    m_step = 0
    if mask is not None:
        mask, q.m_plane, q.m_shared = _arith_operand(mask, a.shape, "arith", "mask")
        m_step = 0 if q.m_shared else h * w * (1 if q.m_plane else c)
    b_step = 0 if q.b_shared else h * w * (1 if q.b_plane else c)
    out = np.empty_like(a)
    for i, m in _batches(n, batch):
        check(lib().mi_blur_run_arith(device, a[i:].ctypes.data, b.ctypes.data + i * b_step, None if mask is None else mask.ctypes.data + i * m_step,
                                      out[i:].ctypes.data, w, h, c, m, C.byref(q)), "mi_blur_run_arith")
    return _unstack(out, rank)


def add(a, b, device: int = 0, batch: int = 0):
    """min(a + b, 255) per byte (preset ADD); shapes as arith()."""
    return arith(a, b, arith_preset("add"), None, device, batch)


def subtract(a, b, device: int = 0, batch: int = 0):
    """max(a - b, 0) per byte (preset SUB); shapes as arith()."""
    return arith(a, b, arith_preset("sub"), None, device, batch)


def absdiff(a, b, device: int = 0, batch: int = 0):
    """|a - b| per byte (preset ABSDIFF); shapes as arith()."""
    return arith(a, b, arith_preset("absdiff"), None, device, batch)


def average(a, b, device: int = 0, batch: int = 0):
    """(a + b + 1) >> 1 per byte (preset AVG); shapes as arith()."""
    return arith(a, b, arith_preset("avg"), None, device, batch)


def minimum(a, b, device: int = 0, batch: int = 0):
    """min(a, b) per byte; shapes as arith()."""
    return arith(a, b, arith_preset("min"), None, device, batch)


def maximum(a, b, device: int = 0, batch: int = 0):
    """max(a, b) per byte; shapes as arith()."""
    return arith(a, b, arith_preset("max"), None, device, batch)


def multiply(a, b, mode: str = "255", device: int = 0, batch: int = 0):
    """mode "255": floor((2 a b + 255) / 510), the product of two shares of 255 rounded once (preset MUL255);
    mode "q7": min((a b + 64) >> 7, 255), b a gain image with 128 = unity (preset MULQ7).  Shapes as arith()."""
    if mode not in ("255", "q7"):
        raise ValueError('multiply: mode is "255" or "q7"')
    return arith(a, b, arith_preset("mul255" if mode == "255" else "mulq7"), None, device, batch)


def add_weighted(a, alpha: float, b, beta: float, gamma: float = 0.0, device: int = 0, batch: int = 0):
    """OpenCV's addWeighted in Q12 (mi_blur_arith_weighted): clamp((wa a + wb b + bias) >> 12) with
    wa = floor(alpha 4096 + 0.5), wb = floor(beta 4096 + 0.5), bias = floor(gamma 4096 + 0.5) + 2048.  |alpha|, |beta| <= 16,
    |gamma| <= 8192.  Shapes as arith()."""
    k = Arith()
    if lib().mi_blur_arith_weighted(float(alpha), float(beta), float(gamma), C.byref(k)) != OK:
        raise ValueError("add_weighted: finite weights, |alpha|, |beta| <= 16 and |gamma| <= 8192")
    return arith(a, b, k, None, device, batch)


def blend(a, b, mask, device: int = 0, batch: int = 0):
    """The blend of a and b through a mask (ARITH_LERP): floor((2 (a m + b (255 - m)) + 255) / 510) per byte, one
    rounding, half up; m = 255 gives a, m = 0 gives b.  mask: shapes as arith()'s operands (a grey mask (H, W) serves
    every image and channel), or one int 0..255 for a constant weight."""
    import numpy as np
    import operator
    if not hasattr(mask, "shape") and not isinstance(mask, (list, tuple)):
        level = operator.index(mask)
        if not 0 <= level <= 255:
            raise ValueError("blend: a constant mask is 0..255")
        stack, _ = _tone_stack(a, "blend")
        mask = np.full(stack.shape[1:3], level, np.uint8)
    return arith(a, b, arith_preset("lerp"), mask, device, batch)


def unsharp_mask(images, sigma: float, amount: float = 1.0, device: int = 0, batch: int = 0):
    """Unsharp masking: clamp(((256 + g) a - g blur(a) + 128) >> 8) with g = floor(amount 256 + 0.5), amount in [0, 16],
    and blur(a) = gaussian_blur(images, sigma): ARITH_LINEAR with wa = 256 + g, wb = -g, bias 128, shift 8."""
    import math
    if not 0.0 <= float(amount) <= 16.0:
        raise ValueError("unsharp_mask: amount in [0, 16]")
    g = int(math.floor(float(amount) * 256.0 + 0.5))
    a = _images(images, "unsharp_mask")
    return arith(a, gaussian_blur(a, sigma, device=device, batch=batch), Arith(ARITH_LINEAR, 256 + g, -g, 128, 8), None, device, batch)


def top_hat(images, ksize=3, device: int = 0, batch: int = 0):
    """White top-hat: max(a - open(a), 0) with open(a) = dilate(erode(a, ksize), ksize): preset SUB of the image and its
    opening.  ksize as erode()."""
    a = _images(images, "top_hat")
    return subtract(a, dilate(erode(a, ksize, device, batch), ksize, device, batch), device, batch)


def black_hat(images, ksize=3, device: int = 0, batch: int = 0):
    """Black top-hat: max(close(a) - a, 0) with close(a) = erode(dilate(a, ksize), ksize): preset SUB of the closing and
    the image.  ksize as erode()."""
    a = _images(images, "black_hat")
    return subtract(erode(dilate(a, ksize, device, batch), ksize, device, batch), a, device, batch)


def difference_of_gaussians(images, sigma1: float, sigma2: float, device: int = 0, batch: int = 0):
    """clamp(gaussian_blur(a, sigma1) - gaussian_blur(a, sigma2) + 128): preset DIFF128 of the two blurs, the signed
    difference around grey."""
    a = _images(images, "difference_of_gaussians")
    return arith(gaussian_blur(a, sigma1, device=device, batch=batch), gaussian_blur(a, sigma2, device=device, batch=batch),
                 arith_preset("diff128"), None, device, batch)


def running_average(acc, frame, shift: int, device: int = 0, batch: int = 0):
    """One step of a running-average background: ((2^shift - 1) acc + frame + 2^(shift - 1)) >> shift, shift in 1..8:
    ARITH_LINEAR with wa = 2^shift - 1, wb = 1, bias = 2^(shift - 1).  Returns the new accumulator."""
    import operator
    shift = operator.index(shift)
    if not 1 <= shift <= 8:
        raise ValueError("running_average: shift in 1..8")
    return arith(acc, frame, Arith(ARITH_LINEAR, (1 << shift) - 1, 1, 1 << (shift - 1), shift), None, device, batch)


def warp_coord(warp: "Warp", X: int, Y: int) -> tuple[int, int, int, int]:
    """(x0, y0, fx, fy) of output pixel (X, Y) under warp's mode and matrix (mi_blur_warp_coord): the unclamped tap
    origin and the weights 0..2047 of the taps x0 + 1 and y0 + 1; nearest gives (xi, yi, 0, 0)."""
    x0, y0, fx, fy = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().mi_blur_warp_coord(C.byref(warp), int(X), int(Y), C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)), "mi_blur_warp_coord")
    return x0.value, y0.value, fx.value, fy.value


def rotation_matrix(center, angle: float, scale: float = 1.0):
    """The forward 2 x 3 matrix of OpenCV's getRotationMatrix2D as nested lists (mi_blur_warp_rotation): angle in
    degrees, positive = counter-clockwise with y pointing down."""
    fwd = (C.c_double * 6)()
    check(lib().mi_blur_warp_rotation(float(center[0]), float(center[1]), float(angle), float(scale), fwd), "mi_blur_warp_rotation")
    return [list(fwd[0:3]), list(fwd[3:6])]


def warp_affine(images, M, dsize=None, mode="bilinear", border="constant", fill: int = 0, inverse: bool = False, device: int = 0, batch: int = 0):
    """Affine warp, numpy in -> numpy out, after OpenCV's warpAffine: M is a real 2 x 3 matrix from input to output
    coordinates (inverse=True: from output to input), pixel (x, y) at integer coordinates (x, y); dsize = (out_w, out_h),
    the input's size by default.  Exact fixed-point bilinear (the matrix in Q16, 11 fraction bits, one final rounding) or
    nearest; border 'constant' (taps outside the image are `fill`) or 'clamp' (include/mi_blur.h has the definition).

    images: (H, W), (H, W, C) or (N, H, W, C) uint8; the result has the same rank with out_h and out_w.  device: HIP
    ordinal, or DEVICE_CPU.  Goes through mi_blur_create / mi_blur_ctx_set_warp / mi_blur_submit / mi_blur_sync."""
    a = _images(images, "warp_affine")
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError("warp_affine: images must not be empty")
    wo, ho = (w, h) if dsize is None else (int(dsize[0]), int(dsize[1]))
    if wo < 1 or ho < 1:
        raise ValueError("warp_affine: dsize is (out_w, out_h), both at least 1")
    if not 0 <= int(fill) <= 255:
        raise ValueError("warp_affine: fill is 0..255")
    wp = Warp.from_matrix(M, wo, ho, mode, border, fill, inverse)
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_warp(wp), (ho, wo))
    return out[0, :, :, 0] if rank == 2 else out[0] if rank == 3 else out


def rotate(images, angle: float, scale: float = 1.0, center=None, dsize=None, mode="bilinear", border="constant", fill: int = 0,
           device: int = 0, batch: int = 0):
    """warp_affine with the matrix of rotation_matrix(center, angle, scale): a rotation by `angle` degrees (positive =
    counter-clockwise) about `center`, by default the image's centre ((W - 1) / 2, (H - 1) / 2), at the input's size."""
    a = _images(images, "rotate")
    h, w = (a.shape[0], a.shape[1]) if a.ndim < 4 else (a.shape[1], a.shape[2])
    if center is None:
        center = ((w - 1) / 2.0, (h - 1) / 2.0)
    return warp_affine(a, rotation_matrix(center, angle, scale), dsize, mode, border, fill, False, device, batch)


def warp_perspective_coord(warp: "WarpPerspective", X: int, Y: int) -> tuple[int, int, int, int]:
    """(x0, y0, fx, fy) of output pixel (X, Y) under warp's mode and homography (mi_blur_warp_perspective_coord): the
    unclamped tap origin (it can reach 2^50) and the weights 0..2047; nearest gives (xi, yi, 0, 0)."""
    x0, y0, fx, fy = C.c_int64(), C.c_int64(), C.c_int(), C.c_int()
    check(lib().mi_blur_warp_perspective_coord(C.byref(warp), int(X), int(Y), C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)), "mi_blur_warp_perspective_coord")
    return x0.value, y0.value, fx.value, fy.value


def perspective_matrix(src_quad, dst_quad):
    """The forward 3 x 3 matrix that takes the four points of src_quad to those of dst_quad, as nested lists, M[2][2] = 1
    (mi_blur_warp_perspective_quad; OpenCV's getPerspectiveTransform).  Each quad: four (x, y) pairs."""
    src = [float(v) for pt in src_quad for v in pt]
    dst = [float(v) for pt in dst_quad for v in pt]
    if len(src) != 8 or len(dst) != 8:
        raise ValueError("perspective_matrix: a quad is four (x, y) points")
    H = (C.c_double * 9)()
    check(lib().mi_blur_warp_perspective_quad((C.c_double * 8)(*src), (C.c_double * 8)(*dst), H), "mi_blur_warp_perspective_quad")
    return [list(H[0:3]), list(H[3:6]), list(H[6:9])]


def warp_perspective(images, M, dsize=None, mode="bilinear", border="constant", fill: int = 0, inverse: bool = False, device: int = 0, batch: int = 0):
    """Perspective warp, numpy in -> numpy out, after OpenCV's warpPerspective: M is a real 3 x 3 matrix from input to
    output coordinates (inverse=True: from output to input); dsize = (out_w, out_h), the input's size by default.  Exact
    fixed-point bilinear (the homography with up to 30 fraction bits, positions rounded to 11, one final rounding) or
    nearest; border 'constant' or 'clamp' (include/mi_blur.h has the definition).  A horizon that crosses the output is
    an error.  images, device, batch and the result as warp_affine()."""
    a = _images(images, "warp_perspective")
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError("warp_perspective: images must not be empty")
    wo, ho = (w, h) if dsize is None else (int(dsize[0]), int(dsize[1]))
    if wo < 1 or ho < 1:
        raise ValueError("warp_perspective: dsize is (out_w, out_h), both at least 1")
    if not 0 <= int(fill) <= 255:
        raise ValueError("warp_perspective: fill is 0..255")
    wp = WarpPerspective.from_matrix(M, wo, ho, mode, border, fill, inverse)
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_warp_perspective(wp), (ho, wo))
    return out[0, :, :, 0] if rank == 2 else out[0] if rank == 3 else out


REMAP_FRAC = 11


def _fixed_map(map, name: str):
    """map as a contiguous int32 array of shape (Ho, Wo, 2); ValueError otherwise."""
    import numpy as np
    m = np.asarray(map)
    if m.dtype != np.int32 or m.ndim != 3 or m.shape[2] != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"{name}: a fixed-point map is an int32 array of shape (Ho, Wo, 2)")
    return np.ascontiguousarray(m)


def remap_map(map_x, map_y):
    """The fixed-point map of two real arrays of one 2-D shape (OpenCV's CV_32FC1 map pair): int32 (Ho, Wo, 2), entry
    (Y, X) = (q(map_x[Y, X]), q(map_y[Y, X])), q(v) = floor(v * 2048 + 0.5) clamped into +-2^30 (mi_blur_remap_from_float).
    A value that is not finite is an error."""
    import numpy as np
    x, y = np.ascontiguousarray(map_x, dtype=np.float32), np.ascontiguousarray(map_y, dtype=np.float32)
    if x.ndim != 2 or x.shape != y.shape or x.size == 0:
        raise ValueError("remap_map: map_x and map_y are two arrays of one shape (Ho, Wo)")
    out = np.empty(x.shape + (2,), dtype=np.int32)
    check(lib().mi_blur_remap_from_float(x.ctypes.data, y.ctypes.data, x.size, out.ctypes.data), "mi_blur_remap_from_float")
    return out


def remap_coord(W: int, H: int, px: int, py: int, mode="bilinear") -> tuple[int, int, int, int]:
    """(x0, y0, fx, fy) of the map entry (px, py) on a W x H image (mi_blur_remap_coord): the clamped tap origin and the
    weights 0..2047 of the taps x0 + 1 and y0 + 1; nearest gives (xi, yi, 0, 0)."""
    r = Remap(1, 1, _resize_mode(mode, "remap"), WARP_CLAMP, 0, 0)
    x0, y0, fx, fy = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().mi_blur_remap_coord(C.byref(r), int(W), int(H), int(px), int(py), C.byref(x0), C.byref(y0), C.byref(fx), C.byref(fy)), "mi_blur_remap_coord")
    return x0.value, y0.value, fx.value, fy.value


def remap_plan(map, width: int, height: int, channels: int, mode="bilinear", border="constant", fill: int = 0, stage_bytes: int = 0) -> dict:
    """What blur_remap_tiled_kernel would do with the tiles of one output image (mi_blur_remap_plan): 'tiled' (eligible by
    shape), and if so 'tiles', 'staged', 'direct', 'empty', 'max_box_bytes', 'max_staged_bytes'."""
    m = _fixed_map(map, "remap_plan")
    r = Remap(m.shape[1], m.shape[0], _resize_mode(mode, "remap"), _warp_border(border), int(fill), int(stage_bytes))
    t = RemapTiles()
    check(lib().mi_blur_remap_plan(m.ctypes.data, int(width), int(height), int(channels), C.byref(r), C.byref(t)), "mi_blur_remap_plan")
    return t.as_dict()


def remap(images, map_x, map_y=None, mode="bilinear", border="constant", fill: int = 0, device: int = 0, batch: int = 0, stage_bytes: int = 0):
    """Remap, numpy in -> numpy out, after OpenCV's remap: output pixel (X, Y) samples the input at (map_x[Y, X],
    map_y[Y, X]), pixel (x, y) at integer coordinates.  map_x: an int32 (Ho, Wo, 2) array is a fixed-point map (11
    fraction bits, map_y None); otherwise map_x and map_y are two real (Ho, Wo) arrays, quantised by remap_map().  Exact
    fixed-point bilinear (one final rounding) or nearest; border 'constant' or 'clamp' (include/mi_blur.h has the
    definition).  images, device, batch and the result as warp_affine(); the output is (Ho, Wo)."""
    import numpy as np
    a = _images(images, "remap")
    if map_y is None:
        m = _fixed_map(map_x, "remap")
    else:
        m = remap_map(map_x, map_y)
    rank = a.ndim
    if rank == 2:
        a = a[None, :, :, None]
    elif rank == 3:
        a = a[None]
    n, h, w, c = a.shape
    if h == 0 or w == 0 or c == 0:
        raise ValueError("remap: images must not be empty")
    if not 0 <= int(fill) <= 255:
        raise ValueError("remap: fill is 0..255")
    ho, wo = m.shape[:2]
    r = Remap(wo, ho, _resize_mode(mode, "remap"), _warp_border(border), int(fill), int(stage_bytes))
    out = _filter_images(a, 1, device, batch, lambda ctx: ctx.set_remap(r, m), (ho, wo))
    return out[0, :, :, 0] if rank == 2 else out[0] if rank == 3 else out


def undistort_map(K, dist, size, new_K=None):
    """The fixed-point undistortion map of a pinhole camera (mi_blur_remap_undistort; OpenCV's initUndistortRectifyMap
    with R = I): K and new_K are (fx, fy, cx, cy) or a 3 x 3 camera matrix, new_K None = K; dist is up to five of
    (k1, k2, p1, p2, k3); size = (out_w, out_h).  int32 (out_h, out_w, 2)."""
    import numpy as np

    def intrinsics(k, name):
        k = np.asarray(k, dtype=np.float64)
        if k.shape == (3, 3):
            k = np.array([k[0, 0], k[1, 1], k[0, 2], k[1, 2]])
        if k.shape != (4,):
            raise ValueError(f"undistort_map: {name} is (fx, fy, cx, cy) or a 3 x 3 camera matrix")
        return (C.c_double * 4)(*k.tolist())
    d = [float(v) for v in np.asarray(dist, dtype=np.float64).reshape(-1)]
    if len(d) > 5:
        raise ValueError("undistort_map: dist is up to five coefficients (k1, k2, p1, p2, k3)")
    d += [0.0] * (5 - len(d))
    wo, ho = int(size[0]), int(size[1])
    if wo < 1 or ho < 1 or wo > RESIZE_MAX_DIM or ho > RESIZE_MAX_DIM:
        raise ValueError("undistort_map: size is (out_w, out_h), both 1..32768")
    out = np.empty((ho, wo, 2), dtype=np.int32)
    check(lib().mi_blur_remap_undistort(intrinsics(K, "K"), (C.c_double * 5)(*d), None if new_K is None else intrinsics(new_K, "new_K"), wo, ho, out.ctypes.data),
          "mi_blur_remap_undistort")
    return out


def undistort(images, K, dist, new_K=None, size=None, mode="bilinear", border="constant", fill: int = 0, device: int = 0, batch: int = 0):
    """remap() through undistort_map(K, dist, size, new_K): OpenCV's undistort.  size = (out_w, out_h), the input's by default."""
    a = _images(images, "undistort")
    h, w = (a.shape[0], a.shape[1]) if a.ndim < 4 else (a.shape[1], a.shape[2])
    return remap(a, undistort_map(K, dist, size or (w, h), new_K), None, mode, border, fill, device, batch)
