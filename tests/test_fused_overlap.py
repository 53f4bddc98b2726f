"""Overlapped fused passes on a real MI355X (-m gpu): with "fused_overlap" > 0 consecutive passes of the fused stream that take
the dynamic tail alternate between two streams, and a pass starts when its predecessor raises a gate word in its tail.  The gate
only moves the moment a pass starts, so everything here is about what must NOT change: every output byte equals the oracle
(the output pool is poisoned first, so stale data cannot pass), every batch is counted in exactly once per pass, polls never
run ahead, the timing harvest covers both streams, and nothing waits for long.  Shapes: the smallest that still take
blur_fused_tail_kernel (>= 8192 tiles)."""
import time

import numpy as np
import pytest

from filter_harness import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64, 3, 1, 9000, 35), (32, 48, 4, 2, 8200, 100)]           # h, w, c, radius, images, batch
FIRST = 11
TAIL, STATIC = b"blur_fused_tail_kernel", b"blur_fused_kernel"
_reference = {}


def reference(O, shape):
    """The oracle's output for a shape's stream: computed once, shared by every test, never written to."""
    if shape not in _reference:
        h, w, c, r, n, _ = shape
        want = O.blur_batch(O.lcg_stream(n, h, w, c, first_index=FIRST), r)
        want.setflags(write=False)
        _reference[shape] = want
    return _reference[shape]


def context(pkg, shape):
    h, w, c, r, n, _ = shape
    ctx = pkg.Context(0, w, h, c, r, max_batch=1, n_slots=1)
    ctx.resident_alloc(n)
    ctx.resident_fill_synthetic(FIRST)
    return ctx


def poison(pkg, L, torch, ctx, shape):
    """0xEE in every byte of the output pool (the blur of a constant image), complete before this returns."""
    h, w, c, r, n, _ = shape
    const_in = torch.full((n, h, w, c), 0xEE, dtype=torch.uint8, device="cuda")
    pkg.check(L.mi_blur_enqueue(const_in.data_ptr(), L.mi_blur_resident_out(ctx.h), w, h, c, r, n, None))
    torch.cuda.synchronize()
    probe = np.zeros((1, h, w, c), np.uint8)
    ctx.resident_download(n - 1, probe.ctypes.data, 1)
    assert (probe == 0xEE).all()


def outputs(ctx, shape):
    h, w, c, _, n, _ = shape
    out = np.zeros((n, h, w, c), np.uint8)
    ctx.resident_download(0, out.ctypes.data, n)
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_back_to_back_passes(pkg, L, O, torch_cuda, shape):
    """Six passes with no sync between them, then one sync; then two synced groups of three with the pool poisoned in between."""
    n, batch = shape[4], shape[5]
    nb = (n + batch - 1) // batch
    want = reference(O, shape)
    with context(pkg, shape) as ctx:
        poison(pkg, L, torch_cuda, ctx, shape)
        for _ in range(6):
            ctx.resident_run_fused(n, batch)
            assert L.mi_blur_last_kernel() == TAIL
        ctx.sync()
        assert ctx.resident_batches_done() == nb
        assert np.array_equal(outputs(ctx, shape), want)
        for group in range(2):
            if group == 1:
                poison(pkg, L, torch_cuda, ctx, shape)
            for _ in range(3):
                ctx.resident_run_fused(n, batch)
            ctx.sync()
            assert ctx.resident_batches_done() == nb, group
        assert np.array_equal(outputs(ctx, shape), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_polls_never_run_ahead(pkg, L, O, torch_cuda, shape):
    """All six passes are queued before the first poll, so every poll is about the same latest pass: the count of its leading
    complete batches is never above the number of batches and never goes down."""
    n, batch = shape[4], shape[5]
    nb = (n + batch - 1) // batch
    with context(pkg, shape) as ctx:
        ctx.resident_run_fused(n, batch); ctx.sync()                       # creates the counters and the poll stream
        for _ in range(6):
            ctx.resident_run_fused(n, batch)
        seen, last = [], 0
        deadline = time.monotonic() + 5.0
        while last < nb:
            assert time.monotonic() < deadline, f"stuck: {last} of {nb} batches after 5 s"
            v = ctx.resident_batches_done()
            assert v <= nb, (v, nb)
            assert v >= last, (v, last, seen[-5:])
            seen.append(v)
            last = v
        ctx.sync()
        assert ctx.resident_batches_done() == nb
        print(f"{len(seen)} polls, {sum(1 for v in seen if v < nb)} of them before the last pass had ended")


@pytest.mark.parametrize("shape", SHAPES)
def test_mixed_queue(pkg, L, O, torch_cuda, shape):
    """Timed and untimed passes, a watched one, a short one on the static kernel, another batch size (the counters are zeroed) and
    the release-ordered count, queued without a sync: after one sync outputs and counts are exact, and nothing waited for long."""
    n, batch = shape[4], shape[5]
    want = reference(O, shape)
    with context(pkg, shape) as ctx:
        poison(pkg, L, torch_cuda, ctx, shape)
        t0 = time.perf_counter()
        try:
            ctx.resident_run_fused(n, batch, timed=True)
            ctx.resident_run_fused(n, batch)
            ctx.resident_run_fused(n, batch, watch=True)
            ctx.resident_run_fused(n, batch)
            ctx.resident_run_fused(n, batch, timed=True)
            ctx.resident_run_fused(1000, batch)
            assert L.mi_blur_last_kernel() == STATIC
            ctx.resident_run_fused(n, batch)
            ctx.resident_run_fused(n, batch)
            ctx.resident_run_fused(n, batch + 1)
            ctx.resident_run_fused(n, batch + 1, timed=True)
            pkg.check(L.mi_blur_set_option(b"fused_release", 1))
            ctx.resident_run_fused(n, batch + 1)
            ctx.resident_run_fused(n, batch + 1)
            assert L.mi_blur_last_kernel() == TAIL
        finally:
            pkg.check(L.mi_blur_set_option(b"fused_release", 0))
        ctx.resident_run_fused(n, batch + 1)
        tm = ctx.sync()
        assert time.perf_counter() - t0 < 5.0, "a gate or a watcher sat out its hard limit"
        assert ctx.resident_batches_done() == (n + batch) // (batch + 1)
        assert ctx.timed_coverage()[0] == 3 and tm["kernel_ms"] > 0
        assert np.array_equal(outputs(ctx, shape), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_plain_launches_between_fused_passes(pkg, L, O, torch_cuda, shape):
    n, batch = shape[4], shape[5]
    nb = (n + batch - 1) // batch
    want = reference(O, shape)
    with context(pkg, shape) as ctx:
        poison(pkg, L, torch_cuda, ctx, shape)
        ctx.resident_run_fused(n, batch)
        ctx.resident_run_fused(n, batch)
        ctx.resident_run(n, 1000)
        ctx.resident_run_fused(n, batch)
        ctx.resident_run_fused(n, batch)
        ctx.sync()
        assert ctx.resident_batches_done() == nb
        assert np.array_equal(outputs(ctx, shape), want)


@pytest.mark.parametrize("shape", SHAPES)
def test_option_off_gives_the_same(pkg, L, O, torch_cuda, shape):
    n, batch = shape[4], shape[5]
    nb = (n + batch - 1) // batch
    want = reference(O, shape)
    got = {}
    try:
        for v in (0, 30, 120):
            pkg.check(L.mi_blur_set_option(b"fused_overlap", v))
            with context(pkg, shape) as ctx:
                poison(pkg, L, torch_cuda, ctx, shape)
                for _ in range(6):
                    ctx.resident_run_fused(n, batch)
                ctx.sync()
                got[v] = (ctx.resident_batches_done(), outputs(ctx, shape))
    finally:
        pkg.check(L.mi_blur_set_option(b"fused_overlap", 30))
    for v, (count, out) in got.items():
        assert count == nb, v
        assert np.array_equal(out, want), v


@pytest.mark.parametrize("shape", SHAPES)
def test_every_pass_timed(pkg, L, O, torch_cuda, shape):
    """The passes' timestamp events lie on two streams: the harvest covers both."""
    n, batch = shape[4], shape[5]
    with context(pkg, shape) as ctx:
        ctx.resident_run_fused(n, batch); ctx.sync()
        ctx.reset_timing()
        for _ in range(5):
            ctx.resident_run_fused(n, batch, timed=True)
        tm = ctx.sync()
        assert ctx.timed_coverage()[0] == 5
        assert tm["kernel_ms"] > 0 and tm["launches"] == 5


@pytest.mark.parametrize("shape", SHAPES)
def test_close_with_passes_in_flight(pkg, L, O, torch_cuda, shape):
    n, batch = shape[4], shape[5]
    ctx = context(pkg, shape)
    for _ in range(6):
        ctx.resident_run_fused(n, batch)
    t0 = time.perf_counter()
    ctx.close()
    assert time.perf_counter() - t0 < 5.0
