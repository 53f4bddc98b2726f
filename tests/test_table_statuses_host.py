"""The status of every enqueue, cpu_run and run export of the families outside Filter (histogram / tone tables, CLAHE,
two-image arithmetic, integral / box, distance transform) for every kind of bad argument, as one table.

Every export answers in the same order: all of its arguments (MI_BLUR_ERR_INVALID), then the empty batch (MI_BLUR_OK),
then the device (MI_BLUR_ERR_NO_DEVICE).  So one rule gives the expected column: a bad argument reads ERR_INVALID with
n_images 1 and with n_images 0; a good call with n_images 0 reads OK on any ordinal; a good call with an image reads OK on
the CPU device and, without a GPU, ERR_NO_DEVICE from every enqueue export and from every run export on ordinals 0, 99
and -2.  With a GPU the good enqueue and the good run on ordinal 0 read OK and nothing else changes.  The table was
recorded from the library before the exports were given one guard and one blocking path, and passes there unchanged.

One shape: 8 x 8 x 3, one image.  Every pointer that is not the null under test is a real buffer of BUF bytes, on the
device for the enqueue rows of the GPU column; a misaligned pointer is such a buffer plus 1 byte (and plus 4 bytes where
the form demands 16: a device table or work buffer)."""
import ctypes as C
import re
import typing

import numpy as np
import pytest

W, H, CH = 8, 8, 3
OK, INVALID, NO_DEVICE = 0, -1, -2
BUF = 1 << 16                                                    # holds every image, table and work buffer of the shape
ORDINALS = (0, 99, -2)
POINTERS = ("i", "b", "m", "o", "t", "q", "lut", "wk")           # in, B, mask, out, table / S, Q, byte tables, work


class Export(typing.NamedTuple):
    kind: str                                                    # "enqueue" | "cpu_run" | "run"
    struct: typing.Optional[str]                                 # the family whose spec struct the export takes
    call: typing.Callable                                        # (L, a) -> status; a: the arguments by name
    pointers: tuple                                              # the pointers that must not be null
    aligned: dict = {}                                           # pointer -> the alignment its form demands
    bad: dict = {}                                               # further invalid combinations: case -> arguments
    cpu: typing.Optional[str] = None                             # run: the cpu_run export of the same bytes


def _p(k):
    return None if k is None else C.byref(k)


def _edit(k, **fields):
    k = type(k).from_buffer_copy(k)
    for name, v in fields.items():
        setattr(k, name, v)
    return k


def _structs(pkg):
    """family -> (a valid spec struct, an invalid one)."""
    tone = pkg.Tone(pkg.TONE_EQUALIZE, 0, 0, 0, 0)
    clahe = pkg.Clahe(2, 2, 512, 0)
    lerp = pkg.arith_preset("lerp")                              # the one operation that takes all three operands
    box = pkg.Box(pkg.BOX_THRESHOLD, 1, 1, 0, 0)                 # from_integral: the one that takes the images
    dist = pkg.Dist(pkg.DIST_L2, 0, 0, pkg.DIST_BYTE, 0)
    return {"tone": (tone, _edit(tone, mode=7)), "clahe": (clahe, _edit(clahe, tiles_x=0)), "arith": (lerp, _edit(lerp, b_plane=2)),
            "box": (box, _edit(box, rx=-1)), "dist": (dist, _edit(dist, metric=3))}


E = Export
EXPORTS = {
    "mi_blur_enqueue_hist": E("enqueue", None, lambda L, a: L.mi_blur_enqueue_hist(a["i"], a["t"], a["w"], a["h"], a["c"], a["n"], None),
                              ("i", "t"), {"t": 16}),
    "mi_blur_cpu_run_hist": E("cpu_run", None, lambda L, a: L.mi_blur_cpu_run_hist(a["i"], a["t"], a["w"], a["h"], a["c"], a["n"], 1),
                              ("i", "t"), {"t": 4}),
    "mi_blur_run_hist": E("run", None, lambda L, a: L.mi_blur_run_hist(a["dev"], a["i"], a["t"], a["w"], a["h"], a["c"], a["n"]),
                          ("i", "t"), {"t": 4}, cpu="mi_blur_cpu_run_hist"),
    "mi_blur_enqueue_tables": E("enqueue", None,
                                lambda L, a: L.mi_blur_enqueue_tables(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], a["lut"], None),
                                ("i", "o", "lut"), bad={"in == out": dict(o="i")}),
    "mi_blur_cpu_run_tables": E("cpu_run", None,
                                lambda L, a: L.mi_blur_cpu_run_tables(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], a["lut"], 1),
                                ("i", "o", "lut"), bad={"in == out": dict(o="i")}),
    "mi_blur_enqueue_tone": E("enqueue", "tone",
                              lambda L, a: L.mi_blur_enqueue_tone(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                              ("i", "o", "wk"), {"wk": 16}, {"in == out": dict(o="i")}),
    "mi_blur_cpu_run_tone": E("cpu_run", "tone",
                              lambda L, a: L.mi_blur_cpu_run_tone(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], 1),
                              ("i", "o"), {"wk": 4}, {"in == out": dict(o="i")}),
    "mi_blur_run_tone": E("run", "tone",
                          lambda L, a: L.mi_blur_run_tone(a["dev"], a["i"], a["o"], a["wk"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                          ("i", "o"), {"wk": 4}, {"in == out": dict(o="i")}, cpu="mi_blur_cpu_run_tone"),
    "mi_blur_enqueue_clahe_tables": E("enqueue", "clahe",
                                      lambda L, a: L.mi_blur_enqueue_clahe_tables(a["i"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                                      ("i", "wk"), {"wk": 16}),
    "mi_blur_enqueue_clahe_apply": E("enqueue", "clahe",
                                     lambda L, a: L.mi_blur_enqueue_clahe_apply(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["lut"], None),
                                     ("i", "o", "lut"), bad={"in == out": dict(o="i")}),
    "mi_blur_enqueue_clahe": E("enqueue", "clahe",
                               lambda L, a: L.mi_blur_enqueue_clahe(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                               ("i", "o", "wk"), {"wk": 16}, {"in == out": dict(o="i")}),
    "mi_blur_cpu_run_clahe_tables": E("cpu_run", "clahe",
                                      lambda L, a: L.mi_blur_cpu_run_clahe_tables(a["i"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], 1),
                                      ("i", "wk"), {"wk": 4}),
    "mi_blur_cpu_run_clahe_apply": E("cpu_run", "clahe",
                                     lambda L, a: L.mi_blur_cpu_run_clahe_apply(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["lut"], 1),
                                     ("i", "o", "lut"), bad={"in == out": dict(o="i")}),
    "mi_blur_cpu_run_clahe": E("cpu_run", "clahe",
                               lambda L, a: L.mi_blur_cpu_run_clahe(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], 1),
                               ("i", "o"), {"wk": 4}, {"in == out": dict(o="i")}),
    "mi_blur_run_clahe": E("run", "clahe",
                           lambda L, a: L.mi_blur_run_clahe(a["dev"], a["i"], a["o"], a["wk"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                           ("i", "o"), {"wk": 4}, {"in == out": dict(o="i")}, cpu="mi_blur_cpu_run_clahe"),
    "mi_blur_enqueue_arith": E("enqueue", "arith",
                               lambda L, a: L.mi_blur_enqueue_arith(a["i"], a["b"], a["m"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), None),
                               ("i", "b", "m", "o")),
    "mi_blur_cpu_run_arith": E("cpu_run", "arith",
                               lambda L, a: L.mi_blur_cpu_run_arith(a["i"], a["b"], a["m"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), 1),
                               ("i", "b", "m", "o")),
    "mi_blur_run_arith": E("run", "arith",
                           lambda L, a: L.mi_blur_run_arith(a["dev"], a["i"], a["b"], a["m"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                           ("i", "b", "m", "o"), cpu="mi_blur_cpu_run_arith"),
    "mi_blur_enqueue_integral": E("enqueue", None,
                                  lambda L, a: L.mi_blur_enqueue_integral(a["i"], a["t"], a["q"], a["w"], a["h"], a["c"], a["n"], a["wk"], None),
                                  ("i", "wk"), {"t": 16, "q": 16, "wk": 16}, {"no table": dict(t=None, q=None)}),
    "mi_blur_cpu_run_integral": E("cpu_run", None,
                                  lambda L, a: L.mi_blur_cpu_run_integral(a["i"], a["t"], a["q"], a["w"], a["h"], a["c"], a["n"], 1),
                                  ("i",), {"t": 4, "q": 4}, {"no table": dict(t=None, q=None)}),
    "mi_blur_run_integral": E("run", None,
                              lambda L, a: L.mi_blur_run_integral(a["dev"], a["i"], a["t"], a["q"], a["w"], a["h"], a["c"], a["n"]),
                              ("i",), {"t": 4, "q": 4}, {"no table": dict(t=None, q=None)}, cpu="mi_blur_cpu_run_integral"),
    "mi_blur_enqueue_box_from_integral": E("enqueue", "box",
                                           lambda L, a: L.mi_blur_enqueue_box_from_integral(a["i"], a["t"], None, a["o"], a["w"], a["h"], a["c"], a["n"],
                                                                                            _p(a["k"]), None),
                                           ("i", "t", "o"), {"t": 16}),
    "mi_blur_enqueue_box": E("enqueue", "box",
                             lambda L, a: L.mi_blur_enqueue_box(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                             ("i", "o", "wk"), {"wk": 16}),
    "mi_blur_cpu_run_box": E("cpu_run", "box", lambda L, a: L.mi_blur_cpu_run_box(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), 1),
                             ("i", "o")),
    "mi_blur_run_box": E("run", "box", lambda L, a: L.mi_blur_run_box(a["dev"], a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                         ("i", "o"), cpu="mi_blur_cpu_run_box"),
    "mi_blur_enqueue_dist": E("enqueue", "dist",
                              lambda L, a: L.mi_blur_enqueue_dist(a["i"], a["t"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                              ("i", "t", "wk"), {"t": 16, "wk": 16}),
    "mi_blur_enqueue_dist_u8": E("enqueue", "dist",
                                 lambda L, a: L.mi_blur_enqueue_dist_u8(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), a["wk"], None),
                                 ("i", "o", "wk"), {"wk": 16}),
    "mi_blur_cpu_run_dist": E("cpu_run", "dist", lambda L, a: L.mi_blur_cpu_run_dist(a["i"], a["t"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), 1),
                              ("i", "t"), {"t": 4}),
    "mi_blur_cpu_run_dist_u8": E("cpu_run", "dist", lambda L, a: L.mi_blur_cpu_run_dist_u8(a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"]), 1),
                                 ("i", "o")),
    "mi_blur_run_dist": E("run", "dist", lambda L, a: L.mi_blur_run_dist(a["dev"], a["i"], a["t"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                          ("i", "t"), {"t": 4}, cpu="mi_blur_cpu_run_dist"),
    "mi_blur_run_dist_u8": E("run", "dist", lambda L, a: L.mi_blur_run_dist_u8(a["dev"], a["i"], a["o"], a["w"], a["h"], a["c"], a["n"], _p(a["k"])),
                             ("i", "o"), cpu="mi_blur_cpu_run_dist_u8"),
}


def _work_fits(pkg, L):
    """Every work buffer of the table's shape fits BUF, and so does every table."""
    s = _structs(pkg)
    sizes = [L.mi_blur_tone_work_bytes(CH, 1), L.mi_blur_clahe_work_bytes(W, H, CH, 1, C.byref(s["clahe"][0])),
             L.mi_blur_integral_work_bytes(W, H, CH, 1, 1), L.mi_blur_box_work_bytes(W, H, CH, 1, C.byref(s["box"][0])),
             L.mi_blur_dist_work_bytes(W, H, CH, 1, C.byref(s["dist"][0])), 4 * CH * 256, 4 * W * H * CH]
    return all(0 < b <= BUF for b in sizes)


def statuses(pkg, L, device, host):
    """{export: {case: status}}: the enqueue rows on the buffers `device` ({pointer: address}), the others on `host`."""
    structs = _structs(pkg)
    got = {}
    for name, e in EXPORTS.items():
        valid, invalid = structs[e.struct] if e.struct else (None, None)
        base = dict(device if e.kind == "enqueue" else host, w=W, h=H, c=CH, n=1, k=valid, dev=0)
        bad = {f"null {p}": {p: None} for p in e.pointers}
        bad.update({"width 0": dict(w=0), "channels 5": dict(c=5), "n_images -1": dict(n=-1)})
        if e.struct:
            bad.update({"invalid struct": dict(k=invalid), "null struct": dict(k=None)})
        for p, align in e.aligned.items():
            bad[f"{p} + 1"] = {p: base[p] + 1}
            if align == 16:
                bad[f"{p} + 4"] = {p: base[p] + 4}
        bad.update({case: {p: base[v] if isinstance(v, str) else v for p, v in f.items()} for case, f in e.bad.items()})
        row = {}
        for case, f in bad.items():
            row[case] = e.call(L, {**base, **f})
            if "n" not in f:
                row[case + ", n_images 0"] = e.call(L, {**base, **f, "n": 0})       # the arguments come before the empty batch
        for dev in ORDINALS if e.kind == "run" else (0,):
            where = f" on ordinal {dev}" if e.kind == "run" else ""
            row["good, n_images 0" + where] = e.call(L, {**base, "n": 0, "dev": dev})
            row["good" + where] = e.call(L, {**base, "dev": dev})
        got[name] = row
    return got


def expected(got, with_gpu):
    """The rule of the module's docstring, for the cases of `got`."""
    want = {}
    for name, row in got.items():
        kind = EXPORTS[name].kind
        launched = OK if with_gpu else NO_DEVICE
        want[name] = {}
        for case in row:
            if not case.startswith("good"):
                want[name][case] = INVALID
            elif "n_images 0" in case or kind == "cpu_run":
                want[name][case] = OK
            elif kind == "enqueue" or case == "good on ordinal 0":
                want[name][case] = launched
            else:
                want[name][case] = NO_DEVICE
    return want


def _host_buffers(rng=None):
    """({pointer: address}, {pointer: array}) of BUF-byte host buffers: random bytes with rng, else zeros."""
    arrays = {p: (rng.integers(0, 256, BUF, dtype=np.uint8) if rng else np.zeros(BUF, np.uint8)) for p in POINTERS}
    return {p: a.ctypes.data for p, a in arrays.items()}, arrays


def _assert_table(got, want):
    assert sorted(got) == sorted(EXPORTS) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_the_table_names_every_export_of_the_five_families(pkg):
    mine = re.compile(r"mi_blur_(enqueue|cpu_run|run)_(hist|tables|tone|clahe|arith|integral|box|dist)\w*")
    declared = [s for s in pkg.declared_symbols() if mine.fullmatch(s)]
    assert sorted(declared) == sorted(EXPORTS) and len(EXPORTS) == 31


def test_statuses_without_a_device(pkg, L):
    if L.mi_blur_device_count() > 0:
        pytest.skip("the column of a machine without a GPU")
    assert _work_fits(pkg, L)
    host, keep = _host_buffers()
    got = statuses(pkg, L, host, host)
    _assert_table(got, expected(got, False))
    assert sum(len(row) for row in got.values()) == 593 and keep


def test_run_on_the_cpu_device_gives_the_bytes_of_cpu_run(pkg, L):
    """mi_blur_run_*(MI_BLUR_DEVICE_CPU) is MI_BLUR_OK and leaves what the matching mi_blur_cpu_run_* leaves, in every
    buffer the call may write: random inputs, every output, table and work buffer filled with 0xA5 first."""
    structs = _structs(pkg)
    assert _work_fits(pkg, L)
    for name, e in EXPORTS.items():
        if e.kind != "run":
            continue
        left = []
        for export in (e, EXPORTS[e.cpu]):
            addr, arrays = _host_buffers(np.random.default_rng(5))
            for p in ("o", "t", "q", "wk"):
                arrays[p][:] = 0xA5
            a = dict(addr, w=W, h=H, c=CH, n=1, k=structs[e.struct][0] if e.struct else None, dev=pkg.DEVICE_CPU)
            assert export.call(L, a) == OK, name
            left.append(np.concatenate([arrays[p] for p in ("o", "t", "q", "wk")]))
        assert np.array_equal(left[0], left[1]) and (left[0] != 0xA5).any(), name


@pytest.mark.gpu
def test_statuses_with_a_device(pkg, L):
    import torch
    assert torch.cuda.is_available() and L.mi_blur_device_count() >= 1
    assert _work_fits(pkg, L)
    tensors = {p: torch.zeros(BUF, dtype=torch.uint8, device="cuda") for p in POINTERS}
    host, keep = _host_buffers()
    got = statuses(pkg, L, {p: t.data_ptr() for p, t in tensors.items()}, host)
    torch.cuda.synchronize()
    _assert_table(got, expected(got, True))
    assert keep
