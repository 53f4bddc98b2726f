"""What sep_down_rate.py, resize_rate.py and warp_rate.py share: the command line, the library under test and rate().

--lib PATH times another build of libmi_blur.so (the mechanism of sched_ab.py: pkg.LIB_PATH is set before pkg.lib()
loads it), so that one session can time the parent's library, this tree's and the parent's again.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def setup():
    """(args, torch, pkg, L) on GPU 0."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--json", default="")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--lib", default="", help="time this libmi_blur.so instead of the tree's")
    args = ap.parse_args()
    import torch
    pkg = entry.load_package()
    if args.lib:
        pkg.LIB_PATH = os.path.abspath(args.lib)
        print(f"library: {pkg.LIB_PATH}")
    L = pkg.lib()
    torch.cuda.set_device(0)
    return args, torch, pkg, L


def rate(torch, go, seconds, ramp, warm=2, probe=3, min_reps=5):
    """(us per call, calls): `warm` calls, `probe` timed ones to size the run, `seconds` of uncounted calls when `ramp`,
    then at least `seconds` (and min_reps) of calls back to back on the current stream between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(warm):
        go()
    e0.record()
    for _ in range(probe):
        go()
    e1.record()
    torch.cuda.synchronize()
    reps = max(min_reps, int(seconds * 1e3 / max(e0.elapsed_time(e1) / probe, 1e-3)) + 1)
    if ramp:
        for _ in range(reps):
            go()
    e0.record()
    for _ in range(reps):
        go()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, reps


def once(torch, *launches):
    """Five launches of each, in order, and nothing else (for a kernel trace)."""
    for go in launches:
        for _ in range(5):
            go()
    torch.cuda.synchronize()


def save(args, rows):
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)
