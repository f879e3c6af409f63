"""the device buffers of the regions calls (csrc/cx_regions.hip) in the manner of tests/test_gpu_watershed_buffers.py, at the size
"small" of tests/buffer_families.py: the four calls at growing and shrinking shapes on one context give what a fresh context gives and
what the restatement gives, a second identical walk allocates nothing, and closing the context gives every byte back."""
import numpy as np
import pytest

import buffer_families as F
import regions_ref as R

pytestmark = pytest.mark.gpu

SMALL = F.SHAPES3["small"]
# growing, shrinking, growing again past the first, back down: every buffer of the state is reused below its capacity and regrown above it
WALK = [(5, 6, 7), SMALL, (3, 3, 3), (SMALL[0] + 2, SMALL[1], SMALL[2] + 9), (9, 10, 70), SMALL]
KINDS = ("voronoi5_zero", "noise", "gaps", "voronoi200", "negative", "voronoi200_zero")
NAMES = ("uint8", "float32", "int16", "bfloat16", "float16", "int8")


def inputs(shape, n):
    L = R.pattern(shape, KINDS[n], seed=n)
    V, name = R.typed_values(shape, NAMES[n], seed=n)
    k = int(max(L.max(), 0))
    keep = (np.arange(k + 1) % 2).astype(np.uint8)
    table = ((np.arange(k + 1) * 5) % 11).astype(np.int32)
    far = tuple(x - 1 for x in shape)
    box = ((far[0] // 2, 0, 1 if far[2] else 0), far)
    return L, V, name, keep, table, box, n % 3


def calls(ctx, shape, n, from_device):
    "the four calls -> [records, pairs, (ones, shape, origin, mask bytes), mapped bytes]"
    import torch
    L, V, name, keep, table, box, pad = inputs(shape, n)
    if from_device:      # from the device; the mask stays in the context, the map goes into a caller's buffer
        tl = torch.from_numpy(L).cuda()
        tv = torch.from_numpy(V.view(np.int16) if V.dtype == np.uint16 else V).cuda()
        res = torch.empty(shape, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        labels = (tl.data_ptr(), shape)
        records = ctx.regions_grid(labels, (tv.data_ptr(), name, shape))
        ones, mshape, origin, ptr = ctx.regions_select(labels, keep, box, pad)
        assert ctx.regions_mask_result() == (mshape, ptr, origin, ones)
        mask = ctx.regions_select(labels, keep, box, pad, download=True)[3]
        ctx.regions_map(labels, table, out=res.data_ptr())
        mapped = res.cpu().numpy()
    else:
        labels = L
        records = ctx.regions_grid(L, (V, name, shape))
        ones, mshape, origin, mask = ctx.regions_select(L, keep, box, pad, download=True)
        mapped = ctx.regions_map(L, table, download=True)
    return [records, ctx.regions_contacts(labels), (ones, mshape, origin, mask.tobytes()), mapped.tobytes()]


def walk(ctx):
    return [calls(ctx, shape, n, n % 2 == 0) for n, shape in enumerate(WALK)]


def same(got, want, name):
    records, pairs, mask, mapped = got
    w_records, w_pairs, w_mask, w_mapped = want
    for field in R.REGION_DTYPE.names:
        if field != "vsum" or name not in R.FLOAT_NAMES:
            assert records[field].tobytes() == w_records[field].tobytes(), field
    # (the values of typed_values add up exactly in double: the float vsum is the same number in any order, NaN where both infinities meet)
    assert np.array_equal(records["vsum"], w_records["vsum"], equal_nan=True)
    assert pairs.tobytes() == w_pairs.tobytes() and mask == w_mask and mapped == w_mapped


def test_growing_and_shrinking_shapes_equal_a_fresh_context_and_the_restatement():
    from contourist_amd import _ffi
    start = _ffi.device_bytes()[0]
    ctx = _ffi.Context()
    try:
        first = walk(ctx)
        held, allocations = _ffi.device_bytes(ctx.handle)
        again = walk(ctx)
        assert _ffi.device_bytes(ctx.handle) == (held, allocations)      # the scratch is reused: a second walk allocates nothing
        # at least the uploaded labels and values of the largest call, its mapped labels and its records
        assert held >= (4 + 1) * int(np.prod(WALK[3]))
        for n, shape in enumerate(WALK):
            L, V, name, keep, table, box, pad = inputs(shape, n)
            sel = R.select_fast(L, keep, box, pad)
            want = [R.regions(L, V, name), R.contacts(L), (sel[2], sel[0].shape, sel[1], sel[0].tobytes()), R.relabel(L, table).tobytes()]
            fresh = _ffi.Context()
            try:
                alone = calls(fresh, shape, n, False)
            finally:
                fresh.close()
            for got in (first[n], again[n], alone):
                same(got, want, name)
    finally:
        ctx.close()
    assert _ffi.device_bytes()[0] == start
