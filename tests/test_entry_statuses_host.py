"""The status of every mi_blur_enqueue*, mi_blur_cpu_run* and mi_blur_ctx_set_* export for every kind of bad argument, as
one table of literals recorded from the library before the exports were given one shared body.

The exports do not check the same things before they ask for a device (the box forms check nothing, the sep forms the
kernel only, ...), so without a GPU some bad arguments read MI_BLUR_ERR_NO_DEVICE and others MI_BLUR_ERR_INVALID.  That
unevenness is observable, so it is pinned here: NO_DEVICE is the column of a machine without a GPU, WITH_DEVICE the
column of one with an MI355X.  One shape: 16 x 8 x 3 (a case that needs another width says so).

No row of the GPU column launches a kernel: each is answered with a negative status, or with MI_BLUR_OK for n_images
== 0 (the setter rows and the mi_blur_cpu_run* rows run on the CPU device).  Every pointer that is not the null under test
is a real buffer of BUF bytes, on the device for the enqueue rows of the GPU column.  Rows that a GPU would answer
with a launch (HOST_ONLY) are in the NO_DEVICE column only."""
import ctypes as C
import typing

import numpy as np
import pytest

W, H, CH = 16, 8, 3
BUF = 1 << 20                                                    # holds the largest image of the table: 32769 x 8 x 3


class Args(typing.NamedTuple):
    i: typing.Any
    o: typing.Any
    w: int = W
    h: int = H
    c: int = CH
    n: int = 1
    y0: int = 0
    y1: int = H
    f: typing.Any = None


def _p(k):
    return None if k is None else C.byref(k)


def _edit(k, **fields):
    k = type(k).from_buffer_copy(k)
    for name, v in fields.items():
        setattr(k, name, v)
    return k


def _families(pkg):
    """family -> (a valid filter, {case: Args fields of an invalid one}).  A filter is what the family's exports take:
    a radius, a struct, an (op, rx, ry) triple, a (SepKernel, Decimation) pair."""
    sep = pkg.SepKernel.from_taps([1, 2, 1])
    lopsided = _edit(sep)
    lopsided.wx[0] = 2                                           # 2 + 2 + 1: not a power of two
    dec = pkg.Decimation(2, 2, 1, 1)
    rs = pkg.Resize(32, 16, pkg.RESIZE_BILINEAR)
    bil = pkg.Bilateral.gauss(0.0, 25.0, 1)
    dark = _edit(bil)
    dark.spatial[4] = 0                                          # the centre of the 3 x 3 table
    conv = pkg.Conv.preset("sharpen")
    return {
        "box": (1, {"radius 0": dict(f=0), "radius 3": dict(f=3)}),
        "sep": (sep, {"radius 17": dict(f=_edit(sep, rx=17)), "taps sum 5": dict(f=lopsided), "null kernel": dict(f=None)}),
        "sep_down": ((sep, dec), {
            "taps sum 5": dict(f=(lopsided, dec)), "stride 5": dict(f=(sep, pkg.Decimation(5, 2, 0, 0))),
            "null kernel": dict(f=(None, dec)), "null decimation": dict(f=(sep, None)),
            "phase outside the image": dict(w=1)}),              # ox = 1 of a 1-pixel row
        "resize": (rs, {"mode 7": dict(f=_edit(rs, mode=7)), "out width 0": dict(f=_edit(rs, out_width=0)), "null resize": dict(f=None),
                        "input wider than MAX_DIM": dict(w=pkg.RESIZE_MAX_DIM + 1)}),
        "median": (1, {"radius 0": dict(f=0), "radius 8": dict(f=8)}),
        "morph": ((pkg.MORPH_ERODE, 1, 1), {"op 3": dict(f=(3, 1, 1)), "rx 17": dict(f=(pkg.MORPH_ERODE, 17, 1))}),
        "bilateral": (bil, {"radius 9": dict(f=_edit(bil, radius=9)), "zero centre": dict(f=dark), "null kernel": dict(f=None)}),
        "conv": (conv, {"mode 5": dict(f=_edit(conv, mode=5)), "rx 8": dict(f=_edit(conv, rx=8)), "null kernel": dict(f=None)}),
    }


# export -> (family, takes n_images, takes a row range, the call)
ENQUEUE = {
    "mi_blur_enqueue": ("box", True, False, lambda L, a: L.mi_blur_enqueue(a.i, a.o, a.w, a.h, a.c, a.f, a.n, None)),
    "mi_blur_enqueue_ex": ("box", True, True, lambda L, a: L.mi_blur_enqueue_ex(a.i, a.o, a.w, a.h, a.c, a.f, a.n, a.y0, a.y1, 0, None)),
    "mi_blur_enqueue_band": ("box", False, True, lambda L, a: L.mi_blur_enqueue_band(a.i, a.o, a.w, a.h, a.c, a.f, a.y0, a.y1, None)),
    "mi_blur_enqueue_band_peer": ("box", False, True,
                                  lambda L, a: L.mi_blur_enqueue_band_peer(a.i, a.o, a.w, a.h, a.c, a.f, a.y0, a.y1, None, None, None)),
    "mi_blur_enqueue_sep": ("sep", True, False, lambda L, a: L.mi_blur_enqueue_sep(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), None)),
    "mi_blur_enqueue_sep_band": ("sep", False, True, lambda L, a: L.mi_blur_enqueue_sep_band(a.i, a.o, a.w, a.h, a.c, a.y0, a.y1, _p(a.f), None)),
    "mi_blur_enqueue_sep_down": ("sep_down", True, False,
                                 lambda L, a: L.mi_blur_enqueue_sep_down(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f[0]), _p(a.f[1]), None)),
    "mi_blur_enqueue_resize": ("resize", True, False, lambda L, a: L.mi_blur_enqueue_resize(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), None)),
    "mi_blur_enqueue_median": ("median", True, False, lambda L, a: L.mi_blur_enqueue_median(a.i, a.o, a.w, a.h, a.c, a.f, a.n, None)),
    "mi_blur_enqueue_median_band": ("median", False, True, lambda L, a: L.mi_blur_enqueue_median_band(a.i, a.o, a.w, a.h, a.c, a.f, a.y0, a.y1, None)),
    "mi_blur_enqueue_morph": ("morph", True, False, lambda L, a: L.mi_blur_enqueue_morph(a.i, a.o, a.w, a.h, a.c, *a.f, a.n, None)),
    "mi_blur_enqueue_morph_band": ("morph", False, True, lambda L, a: L.mi_blur_enqueue_morph_band(a.i, a.o, a.w, a.h, a.c, *a.f, a.y0, a.y1, None)),
    "mi_blur_enqueue_bilateral": ("bilateral", True, False, lambda L, a: L.mi_blur_enqueue_bilateral(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), None)),
    "mi_blur_enqueue_bilateral_band": ("bilateral", False, True,
                                       lambda L, a: L.mi_blur_enqueue_bilateral_band(a.i, a.o, a.w, a.h, a.c, a.y0, a.y1, _p(a.f), None)),
    "mi_blur_enqueue_conv": ("conv", True, False, lambda L, a: L.mi_blur_enqueue_conv(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), None)),
    "mi_blur_enqueue_conv_band": ("conv", False, True, lambda L, a: L.mi_blur_enqueue_conv_band(a.i, a.o, a.w, a.h, a.c, a.y0, a.y1, _p(a.f), None)),
}
CPU_RUN = {
    "mi_blur_cpu_run": ("box", True, False, lambda L, a: L.mi_blur_cpu_run(a.i, a.o, a.w, a.h, a.c, a.f, a.n, 1)),
    "mi_blur_cpu_run_sep": ("sep", True, False, lambda L, a: L.mi_blur_cpu_run_sep(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), 1)),
    "mi_blur_cpu_run_sep_down": ("sep_down", True, False,
                                 lambda L, a: L.mi_blur_cpu_run_sep_down(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f[0]), _p(a.f[1]), 1)),
    "mi_blur_cpu_run_resize": ("resize", True, False, lambda L, a: L.mi_blur_cpu_run_resize(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), 1)),
    "mi_blur_cpu_run_median": ("median", True, False, lambda L, a: L.mi_blur_cpu_run_median(a.i, a.o, a.w, a.h, a.c, a.f, a.n, 1)),
    "mi_blur_cpu_run_morph": ("morph", True, False, lambda L, a: L.mi_blur_cpu_run_morph(a.i, a.o, a.w, a.h, a.c, *a.f, a.n, 1)),
    "mi_blur_cpu_run_bilateral": ("bilateral", True, False, lambda L, a: L.mi_blur_cpu_run_bilateral(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), 1)),
    "mi_blur_cpu_run_conv": ("conv", True, False, lambda L, a: L.mi_blur_cpu_run_conv(a.i, a.o, a.w, a.h, a.c, a.n, _p(a.f), 1)),
}
# setter -> (family, the call); the struct families take null structs, the others have none to give
SETTERS = {
    "mi_blur_ctx_set_kernel": ("sep", lambda L, h, f: L.mi_blur_ctx_set_kernel(h, _p(f))),
    "mi_blur_ctx_set_sep_down": ("sep_down", lambda L, h, f: L.mi_blur_ctx_set_sep_down(h, _p(f[0]), _p(f[1]))),
    "mi_blur_ctx_set_resize": ("resize", lambda L, h, f: L.mi_blur_ctx_set_resize(h, _p(f))),
    "mi_blur_ctx_set_median": ("median", lambda L, h, f: L.mi_blur_ctx_set_median(h, f)),
    "mi_blur_ctx_set_morph": ("morph", lambda L, h, f: L.mi_blur_ctx_set_morph(h, *f)),
    "mi_blur_ctx_set_bilateral": ("bilateral", lambda L, h, f: L.mi_blur_ctx_set_bilateral(h, _p(f))),
    "mi_blur_ctx_set_conv": ("conv", lambda L, h, f: L.mi_blur_ctx_set_conv(h, _p(f))),
}
# Valid calls (a GPU launches them) and an image no buffer of the table holds: the NO_DEVICE column only.
HOST_ONLY = {("mi_blur_enqueue_sep_down", "input wider than MAX_DIM"), ("mi_blur_enqueue_sep_down", "image over INT_MAX bytes"),
             ("mi_blur_enqueue_resize", "image over INT_MAX bytes")}


def launch_statuses(pkg, L, table, d_in, d_out, with_gpu=False):
    """{export: {case: status}} of the enqueue or cpu_run table on the buffers d_in / d_out (addresses)."""
    fams = _families(pkg)
    got = {}
    for name, (fam, batch, band, call) in table.items():
        valid, invalid = fams[fam]
        base = Args(d_in, d_out, f=valid)
        cases = {"null in": dict(i=None), "null out": dict(o=None), "in == out": dict(o=d_in),
                 "width 0": dict(w=0), "rows 0": dict(h=0), "channels 0": dict(c=0)}
        if batch:
            cases.update({"n_images -1": dict(n=-1), "n_images 0": dict(n=0)})
        if band:
            cases.update({"begin -1": dict(y0=-1), "end 9": dict(y1=H + 1), "begin 4 end 4": dict(y0=4, y1=4)})
        cases.update(invalid)
        if table is ENQUEUE and fam in ("sep_down", "resize"):
            cases.update({"input wider than MAX_DIM": dict(w=pkg.RESIZE_MAX_DIM + 1), "image over INT_MAX bytes": dict(w=1 << 28)})
        got[name] = {case: call(L, base._replace(**fields)) for case, fields in cases.items() if not (with_gpu and (name, case) in HOST_ONLY)}
    return got


def setter_statuses(pkg, L):
    """{setter: {case: status}} on CPU-device contexts of the table's shape."""
    fams = _families(pkg)
    img = np.zeros((H, W, CH), np.uint8)
    out = np.zeros(BUF, np.uint8)
    got = {}
    for name, (fam, call) in SETTERS.items():
        valid, invalid = fams[fam]
        nulls = {case: fields["f"] for case, fields in invalid.items() if case.startswith("null")}
        bad = next(fields["f"] for case, fields in invalid.items() if not case.startswith("null") and "f" in fields)
        row = {"null context": call(L, None, valid)}
        with pkg.Context(pkg.DEVICE_CPU, W, H, CH, 1, max_batch=1) as ctx:
            for case, f in nulls.items():
                row[case] = call(L, ctx.h, f)
            row["invalid"] = call(L, ctx.h, bad)
            row["valid"] = call(L, ctx.h, valid)
            ctx.submit(img.ctypes.data, out.ctypes.data, 1)
            ctx.sync()
            row["valid after a submit"] = call(L, ctx.h, valid)
            for case, f in nulls.items():
                row[case + " after a submit"] = call(L, ctx.h, f)
            row["invalid after a submit"] = call(L, ctx.h, bad)
        got[name] = row
    return got


def all_statuses(pkg, L, d_in, d_out, with_gpu):
    """The whole table: the enqueue rows on d_in / d_out, the cpu_run and setter rows on host buffers."""
    h_in, h_out = np.zeros(BUF, np.uint8), np.zeros(BUF, np.uint8)
    got = launch_statuses(pkg, L, ENQUEUE, d_in, d_out, with_gpu)
    got.update(launch_statuses(pkg, L, CPU_RUN, h_in.ctypes.data, h_out.ctypes.data))
    got.update(setter_statuses(pkg, L))
    return got


NO_DEVICE = {
    "mi_blur_enqueue": {"null in": -2, "null out": -2, "in == out": -2, "width 0": -2, "rows 0": -2, "channels 0": -2, "n_images -1": -2,
        "n_images 0": -2, "radius 0": -2, "radius 3": -2},
    "mi_blur_enqueue_ex": {"null in": -2, "null out": -2, "in == out": -2, "width 0": -2, "rows 0": -2, "channels 0": -2, "n_images -1": -2,
        "n_images 0": -2, "begin -1": -2, "end 9": -2, "begin 4 end 4": -2, "radius 0": -2, "radius 3": -2},
    "mi_blur_enqueue_band": {"null in": -2, "null out": -2, "in == out": -2, "width 0": -2, "rows 0": -2, "channels 0": -2, "begin -1": -2,
        "end 9": -2, "begin 4 end 4": -2, "radius 0": -2, "radius 3": -2},
    "mi_blur_enqueue_band_peer": {"null in": -2, "null out": -2, "in == out": -2, "width 0": -2, "rows 0": -2, "channels 0": -2, "begin -1": -2,
        "end 9": -2, "begin 4 end 4": -2, "radius 0": -2, "radius 3": -2},
    "mi_blur_enqueue_sep": {"null in": -2, "null out": -2, "in == out": -2, "width 0": -2, "rows 0": -2, "channels 0": -2, "n_images -1": -2,
        "n_images 0": -2, "radius 17": -1, "taps sum 5": -1, "null kernel": -1},
    "mi_blur_enqueue_sep_band": {"null in": -2, "null out": -2, "in == out": -2, "width 0": -2, "rows 0": -2, "channels 0": -2, "begin -1": -2,
        "end 9": -2, "begin 4 end 4": -2, "radius 17": -1, "taps sum 5": -1, "null kernel": -1},
    "mi_blur_enqueue_sep_down": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": -2, "taps sum 5": -1, "stride 5": -1, "null kernel": -1, "null decimation": -1, "phase outside the image": -1,
        "input wider than MAX_DIM": -2, "image over INT_MAX bytes": -1},
    "mi_blur_enqueue_resize": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": -2, "mode 7": -1, "out width 0": -1, "null resize": -1, "input wider than MAX_DIM": -1, "image over INT_MAX bytes": -1},
    "mi_blur_enqueue_median": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": -2, "radius 0": -1, "radius 8": -1},
    "mi_blur_enqueue_median_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -2,
        "end 9": -2, "begin 4 end 4": -2, "radius 0": -1, "radius 8": -1},
    "mi_blur_enqueue_morph": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": -2, "op 3": -1, "rx 17": -1},
    "mi_blur_enqueue_morph_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -2,
        "end 9": -2, "begin 4 end 4": -2, "op 3": -1, "rx 17": -1},
    "mi_blur_enqueue_bilateral": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1,
        "n_images -1": -1, "n_images 0": -2, "radius 9": -1, "zero centre": -1, "null kernel": -1},
    "mi_blur_enqueue_bilateral_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1,
        "begin -1": -2, "end 9": -2, "begin 4 end 4": -2, "radius 9": -1, "zero centre": -1, "null kernel": -1},
    "mi_blur_enqueue_conv": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": -2, "mode 5": -1, "rx 8": -1, "null kernel": -1},
    "mi_blur_enqueue_conv_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "mode 5": -1, "rx 8": -1, "null kernel": -1},
    "mi_blur_cpu_run": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 0": -1, "radius 3": -1},
    "mi_blur_cpu_run_sep": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 17": -1, "taps sum 5": -1, "null kernel": -1},
    "mi_blur_cpu_run_sep_down": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "taps sum 5": -1, "stride 5": -1, "null kernel": -1, "null decimation": -1, "phase outside the image": -1},
    "mi_blur_cpu_run_resize": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "mode 7": -1, "out width 0": -1, "null resize": -1, "input wider than MAX_DIM": -1},
    "mi_blur_cpu_run_median": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 0": -1, "radius 8": -1},
    "mi_blur_cpu_run_morph": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "op 3": -1, "rx 17": -1},
    "mi_blur_cpu_run_bilateral": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1,
        "n_images -1": -1, "n_images 0": 0, "radius 9": -1, "zero centre": -1, "null kernel": -1},
    "mi_blur_cpu_run_conv": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "mode 5": -1, "rx 8": -1, "null kernel": -1},
    "mi_blur_ctx_set_kernel": {"null context": -1, "null kernel": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null kernel after a submit": -1, "invalid after a submit": -4},
    "mi_blur_ctx_set_sep_down": {"null context": -1, "null kernel": -1, "null decimation": -1, "invalid": -1, "valid": 0,
        "valid after a submit": -4, "null kernel after a submit": -1, "null decimation after a submit": -1, "invalid after a submit": -4},
    "mi_blur_ctx_set_resize": {"null context": -1, "null resize": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null resize after a submit": -1, "invalid after a submit": -4},
    "mi_blur_ctx_set_median": {"null context": -1, "invalid": -1, "valid": 0, "valid after a submit": -4, "invalid after a submit": -4},
    "mi_blur_ctx_set_morph": {"null context": -1, "invalid": -1, "valid": 0, "valid after a submit": -4, "invalid after a submit": -4},
    "mi_blur_ctx_set_bilateral": {"null context": -1, "null kernel": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null kernel after a submit": -4, "invalid after a submit": -4},
    "mi_blur_ctx_set_conv": {"null context": -1, "null kernel": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null kernel after a submit": -4, "invalid after a submit": -4},
}
WITH_DEVICE = {
    "mi_blur_enqueue": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 0": -1, "radius 3": -1},
    "mi_blur_enqueue_ex": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "begin -1": -1, "end 9": -1, "begin 4 end 4": -1, "radius 0": -1, "radius 3": -1},
    "mi_blur_enqueue_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "radius 0": -1, "radius 3": -1},
    "mi_blur_enqueue_band_peer": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "radius 0": -1, "radius 3": -1},
    "mi_blur_enqueue_sep": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 17": -1, "taps sum 5": -1, "null kernel": -1},
    "mi_blur_enqueue_sep_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "radius 17": -1, "taps sum 5": -1, "null kernel": -1},
    "mi_blur_enqueue_sep_down": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "taps sum 5": -1, "stride 5": -1, "null kernel": -1, "null decimation": -1, "phase outside the image": -1},
    "mi_blur_enqueue_resize": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "mode 7": -1, "out width 0": -1, "null resize": -1, "input wider than MAX_DIM": -1},
    "mi_blur_enqueue_median": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 0": -1, "radius 8": -1},
    "mi_blur_enqueue_median_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "radius 0": -1, "radius 8": -1},
    "mi_blur_enqueue_morph": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "op 3": -1, "rx 17": -1},
    "mi_blur_enqueue_morph_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "op 3": -1, "rx 17": -1},
    "mi_blur_enqueue_bilateral": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1,
        "n_images -1": -1, "n_images 0": 0, "radius 9": -1, "zero centre": -1, "null kernel": -1},
    "mi_blur_enqueue_bilateral_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1,
        "begin -1": -1, "end 9": -1, "begin 4 end 4": -1, "radius 9": -1, "zero centre": -1, "null kernel": -1},
    "mi_blur_enqueue_conv": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "mode 5": -1, "rx 8": -1, "null kernel": -1},
    "mi_blur_enqueue_conv_band": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "begin -1": -1,
        "end 9": -1, "begin 4 end 4": -1, "mode 5": -1, "rx 8": -1, "null kernel": -1},
    "mi_blur_cpu_run": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 0": -1, "radius 3": -1},
    "mi_blur_cpu_run_sep": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 17": -1, "taps sum 5": -1, "null kernel": -1},
    "mi_blur_cpu_run_sep_down": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "taps sum 5": -1, "stride 5": -1, "null kernel": -1, "null decimation": -1, "phase outside the image": -1},
    "mi_blur_cpu_run_resize": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "mode 7": -1, "out width 0": -1, "null resize": -1, "input wider than MAX_DIM": -1},
    "mi_blur_cpu_run_median": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "radius 0": -1, "radius 8": -1},
    "mi_blur_cpu_run_morph": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "op 3": -1, "rx 17": -1},
    "mi_blur_cpu_run_bilateral": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1,
        "n_images -1": -1, "n_images 0": 0, "radius 9": -1, "zero centre": -1, "null kernel": -1},
    "mi_blur_cpu_run_conv": {"null in": -1, "null out": -1, "in == out": -1, "width 0": -1, "rows 0": -1, "channels 0": -1, "n_images -1": -1,
        "n_images 0": 0, "mode 5": -1, "rx 8": -1, "null kernel": -1},
    "mi_blur_ctx_set_kernel": {"null context": -1, "null kernel": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null kernel after a submit": -1, "invalid after a submit": -4},
    "mi_blur_ctx_set_sep_down": {"null context": -1, "null kernel": -1, "null decimation": -1, "invalid": -1, "valid": 0,
        "valid after a submit": -4, "null kernel after a submit": -1, "null decimation after a submit": -1, "invalid after a submit": -4},
    "mi_blur_ctx_set_resize": {"null context": -1, "null resize": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null resize after a submit": -1, "invalid after a submit": -4},
    "mi_blur_ctx_set_median": {"null context": -1, "invalid": -1, "valid": 0, "valid after a submit": -4, "invalid after a submit": -4},
    "mi_blur_ctx_set_morph": {"null context": -1, "invalid": -1, "valid": 0, "valid after a submit": -4, "invalid after a submit": -4},
    "mi_blur_ctx_set_bilateral": {"null context": -1, "null kernel": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null kernel after a submit": -4, "invalid after a submit": -4},
    "mi_blur_ctx_set_conv": {"null context": -1, "null kernel": -1, "invalid": -1, "valid": 0, "valid after a submit": -4,
        "null kernel after a submit": -4, "invalid after a submit": -4},
}


def _assert_table(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_statuses_without_a_device(pkg, L):
    if L.mi_blur_device_count() > 0:
        pytest.skip("the column of a machine without a GPU")
    h_in, h_out = np.zeros(BUF, np.uint8), np.zeros(BUF, np.uint8)
    _assert_table(all_statuses(pkg, L, h_in.ctypes.data, h_out.ctypes.data, False), NO_DEVICE)


@pytest.mark.gpu
def test_statuses_with_a_device(pkg, L):
    import torch
    assert torch.cuda.is_available() and L.mi_blur_device_count() >= 1
    d_in, d_out = (torch.zeros(BUF, dtype=torch.uint8, device="cuda") for _ in range(2))
    _assert_table(all_statuses(pkg, L, d_in.data_ptr(), d_out.data_ptr(), True), WITH_DEVICE)
    torch.cuda.synchronize()
