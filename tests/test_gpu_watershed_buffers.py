"""the device buffers of cx_grid_watershed3d (the seventh slot, csrc/cx_watershed.hip) in the manner of tests/test_gpu_buffers.py, at the
size "small" of tests/buffer_families.py: calls at growing and shrinking shapes on one context give what a fresh context gives and what
the restatement gives, a second identical walk allocates nothing, and closing the context gives every byte back."""
import numpy as np
import pytest

import buffer_families as F
import watershed_ref as W
from test_gpu_watershed import EXACT, lakes, three_labels, typed

pytestmark = pytest.mark.gpu

SMALL = F.SHAPES3["small"]
# growing, shrinking, growing again past the first, back down: every buffer of the state is reused below its capacity and regrown above it
WALK = [(5, 6, 7), SMALL, (3, 3, 3), (SMALL[0] + 2, SMALL[1], SMALL[2] + 9), (9, 10, 70), SMALL]


def inputs(shape, n):
    A, _ = typed(("uint8", "float32", "int16")[n % 3], lakes(shape, 60 + n))
    G = (np.random.RandomState(70 + n).uniform(size=shape) < 0.9).astype(np.uint8)
    return A, three_labels(shape, 80 + n), (G if n % 2 else None), dict(connectivity=1 + n % 3, direction=W.DIRECTIONS[n % 2])


def walk(ctx):
    "the calls of WALK on one context -> [(labels, exact stats)]; every second call leaves its result in the context and reads it from there"
    import torch
    out = []
    for n, shape in enumerate(WALK):
        A, M, G, kw = inputs(shape, n)
        if n % 2:
            stats, labels = ctx.watershed_grid(M, G, samples=A, out_host=True, **kw)
            assert ctx.watershed_result()[0] == shape
        else:      # from the device, into a caller's buffer
            ta, tm = torch.from_numpy(A).cuda(), torch.from_numpy(M).cuda()
            res = torch.empty(shape, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            stats, _ = ctx.watershed_grid(tm.data_ptr(), None, samples=(ta.data_ptr(), str(A.dtype), shape), out=res.data_ptr(), **kw)
            labels = res.cpu().numpy()
        out.append((labels, {k: stats[k] for k in EXACT}))
    return out


def test_growing_and_shrinking_shapes_equal_a_fresh_context_and_the_restatement():
    from contourist_amd import _ffi
    start = _ffi.device_bytes()[0]
    ctx = _ffi.Context()
    try:
        first = walk(ctx)
        held, allocations = _ffi.device_bytes(ctx.handle)
        again = walk(ctx)
        assert _ffi.device_bytes(ctx.handle) == (held, allocations)      # the scratch is reused: a second walk allocates nothing
        # at least the words (8 bytes a sample) and the labels of the largest call
        assert held >= 12 * int(np.prod(WALK[3]))
        for n, shape in enumerate(WALK):
            A, M, G, kw = inputs(shape, n)
            want, exact = W.watershed(A, M, G, **kw)
            fresh = _ffi.Context()
            try:
                stats, alone = fresh.watershed_grid(M, G, samples=A, out_host=True, **kw)
            finally:
                fresh.close()
            for labels, counts in (first[n], again[n], (alone, {k: stats[k] for k in EXACT})):
                assert labels.tobytes() == want.tobytes() and counts == exact, (n, shape)
    finally:
        ctx.close()
    assert _ffi.device_bytes()[0] == start
