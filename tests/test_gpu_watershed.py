"""cx_grid_watershed3d (csrc/cx_watershed.hip) against its numpy restatement (tests/watershed_ref.py), byte for byte and with its exact
counts: shapes around the kernel's tile, a lake that spans tiles, corridors that cross the same tile face again and again, a tile that
had settled and is taken over, staircases over a tile's edge and corner, every sample type from the host and from a device tensor,
regions, the routes with no host copy, what a call leaves alone, the error codes, twice the same bytes, and contourist_amd.volume."""
import itertools

import numpy as np
import pytest

import rank_ref as R
import watershed_ref as W

pytestmark = pytest.mark.gpu

# a workgroup owns 8 x 8 x 64 samples (CXW_T0 x CXW_T1 x CXW_T2), the lanes of a wave along the last axis
TILE = (8, 8, 64)
SHAPES = [(TILE[0] + 1, TILE[1] + 2, 1), (TILE[0] + 2, TILE[1] + 1, TILE[2] - 1), (TILE[0] + 1, TILE[1] + 3, TILE[2]), (1, 1, 5), (2, 2, 2), (3, 1, 70),
          (2 * TILE[0] + 1, TILE[1] + 1, 2 * TILE[2] + 2)]
CONNECTIVITIES = (1, 2, 3)
EXACT = ("n_labelled", "n_unreached", "n_ignored", "n_markers")


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def lakes(shape, seed, levels=6):
    "smooth noise quantised to few levels: ties and lakes everywhere -> an integer level per sample"
    import scipy.ndimage as ndi
    rng = np.random.RandomState(seed)
    f = ndi.uniform_filter(rng.uniform(size=shape), size=3, mode="nearest")
    lo, hi = float(f.min()), float(f.max())
    return np.minimum(((f - lo) / max(hi - lo, 1e-9) * levels).astype(np.int64), levels - 1)


def three_labels(shape, seed):
    "labels 1, 2, 3 on random samples, label 2 on several (some of them neighbours where the array has room)"
    rng = np.random.RandomState(seed)
    M = np.zeros(shape, dtype=np.int32)
    n = int(np.prod(shape))
    spots = rng.choice(n, size=min(n, 6), replace=False)
    flat = M.reshape(-1)
    for spot, label in zip(spots, (1, 2, 3, 2, 2, 2)):
        flat[spot] = label
    if n > 8:
        flat[min(int(spots[1]) + 1, n - 1)] = 2
    return M


def typed(name, levels):
    "integer levels as samples of the type -> (numpy array: uint16 bit patterns for bfloat16; the dtype argument of the restatement)"
    if name in R.FLOATS:
        a = (levels * 0.25 - 0.5).astype(np.float32)
        if name == "float16":
            return a.astype(np.float16), None
        if name == "bfloat16":      # (multiples of 0.25 of this size are bfloat16 values)
            return (a.view(np.uint32) >> 16).astype(np.uint16), "bfloat16"
        return a, None
    info = np.iinfo(np.dtype(name))
    top = levels == levels.max()      # both ends of the type among the values
    return np.where(top, info.max, levels + info.min).astype(name), None


def on_device(name, a):
    "a numpy array (uint16 bit patterns for bfloat16) as a device tensor of the type"
    import torch
    if name == "bfloat16":
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a.view(np.int16) if name == "uint16" else a).cuda()


def check(ctx, A, M, region=None, dtype=None, device=None, cost=W.cost_by_relaxation, expected=None, **kw):
    """one flood == the restatement, byte for byte, with its exact counts -> (stats, labels).  device: (samples, markers, region) on the
    device instead of the host arrays; expected: what the restatement gave for these inputs before"""
    want, exact = W.watershed(A, M, region, dtype=dtype, cost=cost, **kw) if expected is None else expected
    if device is None:
        samples = (A, "bfloat16", A.shape) if dtype else A
        stats, got = ctx.watershed_grid(M, region, samples=samples, out_host=True, **kw)
    else:
        stats, got = ctx.watershed_grid(device[1], device[2], samples=device[0], out_host=True, **kw)
    assert got.dtype == np.int32 and got.tobytes() == want.tobytes(), (A.shape, kw, int((got != want).sum()))
    assert {k: stats[k] for k in EXACT} == exact, (A.shape, kw, stats, exact)
    assert 1 <= stats["rounds"] <= A.size + 8 and stats["tile_visits"] >= stats["rounds"] and 1 <= stats["jump_rounds"] <= 32
    return stats, got


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("direction", W.DIRECTIONS)
def test_shapes_around_the_tile(ctx, direction, connectivity):
    labelled = 0
    for n, shape in enumerate(SHAPES):
        A, _ = typed("uint8", lakes(shape, 10 + n))
        stats, got = check(ctx, A, three_labels(shape, 20 + n), direction=direction, connectivity=connectivity)
        labelled += stats["n_labelled"]
        assert stats["n_markers"] >= 2 and stats["n_unreached"] == 0 and stats["n_labelled"] == A.size      # no region: the flood gets everywhere
    assert labelled > 0


def test_a_lake_spanning_tiles(ctx):
    "a constant relief: the geodesic Voronoi split of the box, exact ties by the index rule, across tile faces"
    shape = (TILE[0] + 1, TILE[1] + 1, 3 * TILE[2])
    A = np.full(shape, 7, dtype=np.uint8)
    M = np.zeros(shape, dtype=np.int32)
    spots = {1: (0, 0, 0), 2: (shape[0] - 1, shape[1] - 1, shape[2] - 1), 3: (4, 4, shape[2] // 2)}
    for label, at in spots.items():
        M[at] = label
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1)
    for connectivity, direction in itertools.product(CONNECTIVITIES, W.DIRECTIONS):
        stats, got = check(ctx, A, M, connectivity=connectivity, direction=direction)
        assert stats["rounds"] >= 2 and stats["n_labelled"] == A.size
        # where one marker is strictly nearest in the metric of the connectivity (a box has no obstacles), the sample is its own
        d = np.sort(np.abs(grid[None] - np.array(list(spots.values()))[:, None, None, None, :]), axis=-1)[..., ::-1]      # per axis, descending
        steps = {1: d.sum(-1), 2: np.maximum(d[..., 0], (d.sum(-1) + 1) // 2), 3: d[..., 0]}[connectivity]
        order = np.sort(steps, axis=0)
        unique = order[0] < order[1]
        assert np.array_equal(got[unique], (np.argmin(steps, axis=0) + 1)[unique]) and unique.mean() > 0.9 and not unique.all()
        assert set(np.unique(got)) == {1, 2, 3}


def corridor_along_axis2(shape):
    "a corridor one sample wide in the plane i = 1: along axis 2 in every second row, turning at alternating ends -> its cells in order"
    cells = []
    for n, j in enumerate(range(0, shape[1], 2)):
        ks = list(range(shape[2])) if n % 2 == 0 else list(range(shape[2] - 1, -1, -1))
        cells += [(1, j, k) for k in ks]
        if j + 2 < shape[1]:
            cells.append((1, j + 1, ks[-1]))
    return cells


def region_of(shape, cells):
    G = np.zeros(shape, dtype=np.uint8)
    G[tuple(np.array(cells).T)] = 1
    return G


@pytest.mark.parametrize("plane", ["along axis 2", "in the (0, 1) plane"])
def test_a_serpentine_corridor_through_nine_tiles(ctx, plane):
    if plane == "along axis 2":
        shape = (3, 2 * TILE[1] + 1, 2 * TILE[2] + 2)
        cells = corridor_along_axis2(shape)
    else:      # the same corridor with the axes turned: rows along axis 1 in the plane k = 1
        shape = (2 * TILE[0] + 1, 2 * TILE[1] + 2, 3)
        cells = [(j, k, i) for i, j, k in corridor_along_axis2((3, shape[0], shape[1]))]
    assert int(np.prod([-(-n // t) for n, t in zip(shape, TILE)])) == 9 and len(set(cells)) == len(cells)
    G = region_of(shape, cells)
    A = np.full(shape, 3, dtype=np.uint8)
    # a marker at each end: the corridor is split in its middle, everything else is outside
    M = np.zeros(shape, dtype=np.int32)
    M[cells[0]], M[cells[-1]] = 1, 2
    stats, got = check(ctx, A, M, G, cost=W.cost_by_heap)
    half = len(cells) // 2
    assert all(got[c] == 1 for c in cells[:half - 1]) and all(got[c] == 2 for c in cells[half + 1:]) and stats["n_labelled"] == len(cells)
    # one marker at one end: d grows to the corridor's length, the chain of pointers is that long
    for end in (cells[0], cells[-1]):
        M = np.zeros(shape, dtype=np.int32)
        M[end] = 5
        stats, got = check(ctx, A, M, G, cost=W.cost_by_heap, direction="falling")
        assert np.array_equal(got, 5 * G.astype(np.int32)) and stats["n_unreached"] == 0
        assert stats["jump_rounds"] >= 2 and stats["rounds"] > 9      # (a pass in place may more than double; every face crossed costs a round)
    # a wall in the middle: what lies behind it is inside the domain and unreached
    G[cells[half]] = 0
    stats, got = check(ctx, A, M, G, cost=W.cost_by_heap)
    assert stats["n_unreached"] == half and stats["n_labelled"] == len(cells) - half - 1


def test_a_tile_that_settled_is_opened_again(ctx):
    """a marker on high ground claims its tile at once; the flood of a far marker on low ground comes down a channel rounds later and
    takes the channel and what climbs out of it first"""
    shape = (3, 3, 3 * TILE[2] + 8)
    A = np.full(shape, 10, dtype=np.uint8)
    A[1, 1, :] = 1
    M = np.zeros(shape, dtype=np.int32)
    M[1, 1, 0], M[0, 0, shape[2] - 1] = 1, 2
    for connectivity in CONNECTIVITIES:
        stats, got = check(ctx, A, M, connectivity=connectivity)
        assert stats["rounds"] >= 4 and (got[1, 1, :] == 1).all() and got[0, 0, -1] == 2 and (got[:, :, -TILE[2]:] == 1).sum() > TILE[2]
    stats, got = check(ctx, 255 - A, M, direction="falling")
    assert (got[1, 1, :] == 1).all()


@pytest.mark.parametrize("needs", [2, 3])
def test_diagonal_staircases(ctx, needs):
    "every step differs on `needs` axes, and the step in the middle leaves the tile over its edge (2) or its corner (3)"
    if needs == 2:
        shape = (3, 2 * TILE[1] + 1, 2 * TILE[2] + 2)
        cells = [(1, d, TILE[2] - TILE[1] + d) for d in range(2 * TILE[1] + 1)]
    else:
        shape = (2 * TILE[0] + 1, 2 * TILE[1] + 1, 2 * TILE[2] + 2)
        cells = [(d, d, TILE[2] - TILE[1] + d) for d in range(2 * TILE[1] + 1)]
    assert (TILE[0] - 1 if needs == 3 else 1, TILE[1] - 1, TILE[2] - 1) in cells
    G = region_of(shape, cells)
    A, _ = typed("int16", lakes(shape, 3))
    for end, connectivity in itertools.product((cells[0], cells[-1]), CONNECTIVITIES):
        M = np.zeros(shape, dtype=np.int32)
        M[end] = 9
        stats, got = check(ctx, A, M, G, connectivity=connectivity, cost=W.cost_by_heap)
        assert stats["n_labelled"] == (len(cells) if connectivity >= needs else 1)
        assert stats["n_unreached"] == (0 if connectivity >= needs else len(cells) - 1)


SPECIALS = np.array([0.0, -0.0, -0.0, 0.0, np.inf, np.nan, -np.inf, 1.0, -np.inf, -np.inf, np.nan, 0.25, np.inf, np.inf, -0.0, 0.0], dtype=np.float32)


@pytest.mark.parametrize("name", R.TYPES)
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    import recon_ref
    shape = (9, 10, 70)
    A, dtype = typed(name, lakes(shape, 9))
    M = three_labels(shape, 31)
    if name in R.FLOATS:      # -0.0 beside +0.0, the infinities as ordinary levels, NaN as walls, a marker on a NaN
        S = SPECIALS.astype(np.float16) if name == "float16" else (recon_ref.round_bfloat16(SPECIALS.astype(np.float64)) if dtype else SPECIALS)
        A[4, 5, 10:10 + len(S)] = S
        A[2, :, 40] = S[5]      # a wall of NaN with one gap
        A[2, 3, 40] = S[0]
        M[4, 5, 15], M[4, 5, 11], M[4, 5, 22] = 3, 1, 2
    G = (np.random.RandomState(2).uniform(size=shape) < 0.85).astype(np.uint8)
    G[tuple(np.argwhere(M == 1)[0])] = 0      # a marker outside the region
    ta, tm, tg = on_device(name, A), torch.from_numpy(M).cuda(), torch.from_numpy(G).cuda()
    torch.cuda.synchronize()
    for direction, connectivity, region in itertools.product(W.DIRECTIONS, (1, 3), (None, G)):
        kw = dict(direction=direction, connectivity=connectivity)
        expected = W.watershed(A, M, region, dtype=dtype, **kw)
        stats, got = check(ctx, A, M, region, dtype=dtype, expected=expected, **kw)
        dev = ((ta.data_ptr(), name, shape), tm.data_ptr(), None if region is None else tg.data_ptr())
        check(ctx, A, M, region, dtype=dtype, device=dev, expected=expected, **kw)
        assert stats["n_ignored"] >= (1 if region is not None else 0) + (1 if name in R.FLOATS else 0)
        if name in R.FLOATS and region is None:
            assert stats["n_ignored"] == 1 and got[4, 5, 15] == 0 and (got[2, :, 40] > 0).sum() == 1


def test_minus_zero_and_the_infinities_are_levels(ctx):
    "rising: +0.0 is a climb from -0.0, so the flood from -0.0 takes every -0.0 first; -inf is the lowest level and +inf the highest"
    Z = np.array([-0.0, -0.0, 0.0, -0.0, -np.inf, np.inf, 1.0, -np.inf], dtype=np.float32).reshape(1, 1, 8)
    M = np.zeros(Z.shape, dtype=np.int32)
    M[0, 0, 0], M[0, 0, 7] = 1, 2
    stats, got = check(ctx, Z, M)
    # from the left: (-0, 0) (-0, 1) (+0, 0) (+0, 1) (+0, 2) (+inf, 0); from the right: (-inf, 0) (1, 0) (+inf, 0).  Both floods wet the +inf sample
    # at (+inf, 0); it takes the label of its neighbour of least W, and (+0, 2) on its left is below (1, 0) on its right
    assert got.reshape(-1).tolist() == [1, 1, 1, 1, 1, 1, 2, 2]
    # falling, +inf lowest and -inf highest.  From the left: (-0, 0) (-0, 1) (-0, 2) (-0, 3) (-inf, 0) (-inf, 1) (-inf, 2); from the right:
    # (-inf, 0) (-inf, 1) (-inf, 2) (-inf, 3)
    stats, got = check(ctx, Z, M, direction="falling")
    assert got.reshape(-1).tolist() == [1, 1, 1, 1, 1, 1, 2, 2]


def test_regions_with_holes_markers_outside_none_and_everywhere(ctx):
    shape = (TILE[0] + 2, TILE[1] + 3, TILE[2] + 5)
    rng = np.random.RandomState(6)
    A, _ = typed("uint8", lakes(shape, 4))
    G = (rng.uniform(size=shape) < 0.7).astype(np.uint8) * 3      # any non-zero byte is inside
    M = three_labels(shape, 5)
    M[0, 0, 0], G[0, 0, 0] = 7, 0      # a marker outside the region
    for connectivity in CONNECTIVITIES:
        stats, got = check(ctx, A, M, G, connectivity=connectivity)
        assert stats["n_ignored"] >= 1 and (got[G == 0] == 0).all() and 7 not in got
    assert stats["n_unreached"] == 0 and check(ctx, A, M, G, connectivity=1)[0]["n_unreached"] > 0      # connectivity 1 leaves islands
    # no markers at all, and none inside the domain: CX_OK, all zeros
    none = np.zeros(shape, dtype=np.int32)
    stats, got = check(ctx, A, none, G)
    assert not got.any() and stats["n_unreached"] == int((G != 0).sum()) and stats["n_markers"] == 0
    only_outside = np.where(G == 0, 4, 0).astype(np.int32)
    stats, got = check(ctx, A, only_outside, G, direction="falling")
    assert not got.any() and stats["n_ignored"] == int((G == 0).sum())
    # every sample a marker (and values that are no labels): everybody keeps its own
    everywhere = rng.randint(-2, 50, size=shape).astype(np.int32)
    stats, got = check(ctx, A, everywhere, connectivity=3)
    assert stats["n_markers"] == int((everywhere > 0).sum())
    everywhere = np.maximum(everywhere, 1)
    assert np.array_equal(check(ctx, A, everywhere)[1], everywhere)
    # labels at the top of int32
    big = three_labels(shape, 8) * (2 ** 31 - 1)
    assert check(ctx, A, big.astype(np.int32))[1].max() == 2 ** 31 - 1


def test_misaligned_inputs_callers_output_and_host_copy(ctx):
    import torch
    from contourist_amd import _ffi
    shape = (5, 9, 67)
    n = int(np.prod(shape))
    rng = np.random.RandomState(12)
    for name in ("uint8", "int16", "float32"):
        flat, dtype = typed(name, lakes((1, 1, n + 1), 30).reshape(-1))
        mflat = np.concatenate([[0], three_labels(shape, 2).reshape(-1)]).astype(np.int32)
        gflat = (rng.uniform(size=n + 1) < 0.9).astype(np.uint8)
        ta, tm, tg = on_device(name, flat)[1:], torch.from_numpy(mflat).cuda()[1:], torch.from_numpy(gflat).cuda()[1:]      # one element off their allocations
        assert ta.data_ptr() % 16 != 0 and tm.data_ptr() % 16 == 4 and tg.data_ptr() % 16 == 1
        A, M, G = flat[1:].reshape(shape), mflat[1:].reshape(shape), gflat[1:].reshape(shape)
        want, exact = W.watershed(A, M, G, connectivity=2, dtype=dtype)
        out = torch.full((n + 2,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        host_out = np.empty(shape, dtype=np.int32)
        stats, got = ctx.watershed_grid(tm.data_ptr(), tg.data_ptr(), 2, samples=(ta.data_ptr(), name, shape), out=out[1:].data_ptr(), out_host=host_out)
        torch.cuda.synchronize()
        raw = out.cpu().numpy()
        assert raw[0] == 0x5A5A5A5A and raw[-1] == 0x5A5A5A5A      # nothing written around the result
        assert raw[1:-1].tobytes() == want.tobytes() and got is host_out and host_out.tobytes() == want.tobytes()
        assert {k: stats[k] for k in EXACT} == exact
        with pytest.raises(_ffi.CxError) as e:      # with an output of the caller's the context holds no result
            ctx.watershed_result()
        assert e.value.code == _ffi.CX_ERR_STATE


def test_pending_results_as_inputs_without_a_host_copy():
    import distance_ref
    import label_ref
    import recon_ref
    import torch
    from contourist_amd import _ffi
    rng = np.random.RandomState(5)
    shape = (9, 10, 70)
    A = (rng.standard_normal(shape) * 3.0).astype(np.float32)
    D = distance_ref.distance(A, 1.5, "above")      # inside {f >= 1.5}
    X = recon_ref.reconstruct(D, "step", connectivity=3, out_kind="changed")[0]
    labels, k = label_ref.label(X, 0.5, "high", 3)
    obj, _ = label_ref.label(A, 1.5, "high", 3)
    region = (obj > 0).astype(np.uint8)
    assert k > 3
    c = _ffi.Context()
    try:
        # distance's pending field as relief, label's pending labels as markers, the pending select mask as region
        k_obj, _ = c.label_grid(1.5, "high", 3, samples=A)
        _, gptr = c.label_select(np.concatenate([[0], np.ones(k_obj)]))
        _, dptr = c.distance_grid(1.5, "above", "float32", samples=A)
        _, xptr = c.reconstruct_grid("step", connectivity=3, out_kind="changed", samples=(dptr, "float32", shape))
        got_k, lptr = c.label_grid(0.5, "high", 3, samples=(xptr, "uint8", shape))
        assert got_k == k
        want, exact = W.watershed(D, labels, region, connectivity=3, direction="falling")
        stats, got = c.watershed_grid(lptr, gptr, 3, "falling", samples=(dptr, "float32", shape), out_host=True)
        assert got.tobytes() == want.tobytes() and {n: stats[n] for n in EXACT} == exact
        # all three are still what they were; the labels wait in the context
        assert c.distance_result()[1] == dptr and c.label_result()[1] == lptr and c.label_mask_result()[1] == gptr
        assert c.watershed_result() == (shape, c.watershed_grid(lptr, gptr, 3, "falling", samples=(dptr, "float32", shape))[1])
        # the pending result as the markers of the next call: the flood of its labels over another relief, into the context again
        B, _ = typed("uint8", lakes(shape, 77))
        tb = torch.from_numpy(B).cuda()
        torch.cuda.synchronize()
        seeds = np.where(rng.uniform(size=shape) < 0.05, want, 0).astype(np.int32)
        _, sptr = c.watershed_grid(seeds, samples=D, direction="falling")      # (host inputs: the pending labels are `seeds` flooded over D)
        first = W.watershed(D, seeds, direction="falling")[0]
        assert c.watershed_result() == (shape, sptr)
        stats, got = c.watershed_grid(sptr, samples=(tb.data_ptr(), "uint8", shape), out_host=True)      # (a host copy does not consume the result)
        wptr = c.watershed_result()[1]
        assert wptr != sptr and got.tobytes() == W.watershed(B, first)[0].tobytes() and stats["n_markers"] == first.size
        back = c.watershed_grid(wptr, samples=(tb.data_ptr(), "uint8", shape), out_host=True)[1]      # every sample a marker: the labels flood to themselves
        assert back.tobytes() == got.tobytes() and c.watershed_result()[1] != wptr
        # the bound grid as relief
        c.upload_grid(A)
        tm = torch.from_numpy(labels).cuda()
        torch.cuda.synchronize()
        stats, got = c.watershed_grid(tm.data_ptr(), out_host=True)
        assert got.tobytes() == W.watershed(A, labels)[0].tobytes()
    finally:
        c.close()


def test_what_a_call_leaves_alone():
    from contourist_amd import _ffi
    rng = np.random.RandomState(19)
    A = (rng.standard_normal((12, 13, 70)) * 3.0).astype(np.float32)
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)      # the other six pending results (label: the labels and the mask)
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        c.label_select(np.arange(k + 1) % 2)
        mask = c.label_mask_result()
        c.resample_grid(np.diag([1.0, 0.5, 1.0]), np.zeros(3), A.shape)
        res = c.resample_result()
        _, qptr = c.rank_grid(3, 13)
        _, rptr = c.reconstruct_grid("shift", h=2.5, connectivity=2)
        stats, wptr = c.watershed_grid(lptr)      # of the bound grid, label's pending labels as markers, into the context
        assert stats["n_markers"] > 0 and c.watershed_result() == (A.shape, wptr)
        c.watershed_grid(three_labels((5, 6, 7), 1), samples=typed("uint8", lakes((5, 6, 7), 1))[0], out_host=True)      # of other samples
        assert c.watershed_result()[0] == (5, 6, 7)
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts      # the grid is the one uploaded
        assert (c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k) and c.label_mask_result() == mask
                and c.resample_result() == res and c.rank_result() == (A.shape, qptr, "float32") and c.reconstruct_result() == (A.shape, rptr, "float32", "values"))
        # and their contents: the reconstruction read back through a rank filter of one sample
        import recon_ref
        same = c.rank_grid(1, 0, samples=(rptr, "float32", A.shape), download=True)[1]
        assert R.same_bytes(same, recon_ref.reconstruct(A, "shift", h=2.5, connectivity=2)[0])
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import torch
    from contourist_amd import _ffi
    shape = (4, 5, 6)
    A, _ = typed("uint8", lakes(shape, 21))
    M = three_labels(shape, 22)
    fresh = _ffi.Context()
    try:
        for call in (lambda: fresh.watershed_grid(M), fresh.watershed_result):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
        tm0 = torch.from_numpy(M).cuda()
        torch.cuda.synchronize()
        assert fresh.lib.cx_grid_watershed3d(fresh.handle, None, 0, 1, 0, 0, 0, tm0.data_ptr(), None, 1, 0, None, None, None) == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    big = torch.zeros(16 * A.size, dtype=torch.uint8, device="cuda")
    n = A.size
    a_in, m_in, g_in = big[4 * n:5 * n], big[6 * n:10 * n], big[11 * n:12 * n]
    a_in.copy_(torch.from_numpy(A).reshape(-1))
    m_in.copy_(torch.from_numpy(M.view(np.uint8).reshape(-1)))
    g_in.fill_(1)
    torch.cuda.synchronize()
    call = ctx.lib.cx_grid_watershed3d

    def raw(relief=None, dtype=1, shape=shape, markers=m_in.data_ptr(), region=None, connectivity=1, direction=0, out=None, handle=None):
        return call(ctx.handle if handle is None else handle, a_in.data_ptr() if relief is None else relief, dtype, 1, shape[0], shape[1], shape[2], markers, region,
                    connectivity, direction, out, None, None)

    assert raw() == _ffi.CX_OK and raw(region=g_in.data_ptr(), connectivity=3, direction=1) == _ffi.CX_OK
    for bad in (dict(dtype=7), dict(dtype=-1), dict(shape=(0, 5, 6)), dict(shape=(4, -1, 6)), dict(markers=None), dict(connectivity=0), dict(connectivity=4),
                dict(direction=2), dict(direction=-1), dict(out=big[12 * n:].data_ptr() + 1), dict(out=big[12 * n:].data_ptr() + 2)):
        assert raw(**bad) == _ffi.CX_ERR_INVALID, bad
    assert call(None, a_in.data_ptr(), 1, 1, 4, 5, 6, m_in.data_ptr(), None, 1, 0, None, None, None) == _ffi.CX_ERR_INVALID
    for many in ((1 << 16, 1 << 16, 1), (1 << 11, 1 << 11, (1 << 9) + 1), (1 << 32, 1, 1)):      # more than 2^31 samples
        assert raw(shape=many) == _ffi.CX_ERR_UNSUPPORTED
    # an output that overlaps the relief, the markers or the region: its first byte, its last, the int32 in front of it
    for inner, size in ((a_in, n), (m_in, 4 * n), (g_in, n)):
        for out in (inner.data_ptr(), inner.data_ptr() + size - 4, inner.data_ptr() - 4 * n + 4):
            assert raw(region=g_in.data_ptr(), out=out) == _ffi.CX_ERR_INVALID
    assert raw(out=g_in.data_ptr() - 4 * n + 4) == _ffi.CX_ERR_INVALID      # (it reaches into the markers)
    # next to them is fine
    assert raw(region=g_in.data_ptr(), out=big[12 * n:].data_ptr()) == _ffi.CX_OK
    ctx.synchronize()
    got = big[12 * n:16 * n].cpu().numpy().view(np.int32).reshape(shape)
    assert got.tobytes() == W.watershed(A, M)[0].tobytes()


def test_twice_the_same_bytes_and_counts(ctx):
    "2^16 samples, 16 tiles: the tiles of a launch race, the result does not"
    shape = (16, 32, 128)
    rng = np.random.RandomState(12)
    A, _ = typed("float32", lakes(shape, 12, levels=9))
    M = np.where(rng.uniform(size=shape) < 2e-3, rng.randint(1, 9, size=shape), 0).astype(np.int32)
    G = (rng.uniform(size=shape) < 0.9).astype(np.uint8)
    for kw in (dict(connectivity=1), dict(connectivity=3, direction="falling"), dict(connectivity=2, region=G)):
        region = kw.pop("region", None)
        stats, got = check(ctx, A, M, region, **kw)
        ctx.watershed_grid(three_labels((3, 3, 3), 1), samples=np.zeros((3, 3, 3), np.uint8), out_host=True)      # (the scratch is reused in between)
        stats2, again = ctx.watershed_grid(M, region, samples=A, out_host=True, **kw)
        assert again.tobytes() == got.tobytes() and all(stats[k] == stats2[k] for k in EXACT)


def two_balls():
    shape = (24, 24, 40)
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).astype(np.float64)
    inside = np.zeros(shape, dtype=bool)
    for centre in ((12, 12, 13), (12, 12, 27)):
        inside |= ((g - np.array(centre)) ** 2).sum(-1) <= 9.0 ** 2
    return inside.astype(np.float32)


def test_volume_split_touching_two_balls():
    import distance_ref
    import label_ref
    import recon_ref
    import torch
    from contourist_amd import volume
    A = two_balls()
    obj = A >= 0.5
    assert volume.label(A, 0.5)[1] == 1
    D = distance_ref.distance(A, 0.5, "above")
    for connectivity in (1, 3):
        H = recon_ref.reconstruct(D, "shift", h=1.0, connectivity=connectivity)[0]
        X = recon_ref.reconstruct(H, "step", connectivity=connectivity, out_kind="changed")[0]
        markers, k = label_ref.label(X, 0.5, "high", connectivity)
        want = W.watershed(D, markers, obj, connectivity=connectivity, direction="falling")[0]
        got = volume.split_touching(A, 0.5, 1.0, connectivity=connectivity)
        got_t = volume.split_touching(torch.from_numpy(A).cuda(), 0.5, 1.0, connectivity=connectivity)
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.tobytes() == want.tobytes()
        assert got_t.is_cuda and got_t.dtype == torch.int32 and got_t.cpu().numpy().tobytes() == want.tobytes()
        # two objects; the cut lies within one sample of the plane between the centres; every object sample is labelled, nothing outside is
        assert set(np.unique(got)) == {0, 1, 2} and np.array_equal(got > 0, obj)
        left, right = got[:, :, :20], got[:, :, 21:]
        assert len(set(np.unique(left[left > 0]))) == 1 and len(set(np.unique(right[right > 0]))) == 1 and left.max() != right.max()
    # side "low": the same objects as the low side of the negated samples
    low = volume.split_touching(-A, -0.25, 1.0, side="low")
    assert np.array_equal(low, volume.split_touching(A, 0.5, 1.0))


def test_volume_watershed_numpy_tensor_and_fewer_dimensions():
    import label_ref
    import recon_ref
    import torch
    from contourist_amd import volume
    shape = (9, 13, 70)
    rng = np.random.RandomState(3)
    A, _ = typed("float32", lakes(shape, 41))
    M = three_labels(shape, 42)
    G = rng.uniform(size=shape) < 0.8

    def both(kw, args, want, stats=None):
        got = volume.watershed(*args, **kw)
        got_t = volume.watershed(*[None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args], **kw)
        if stats is not None:
            (got, s), (got_t, s_t) = got, got_t
            assert {k: s[k] for k in EXACT} == stats == {k: s_t[k] for k in EXACT}
        assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == want.shape and got.tobytes() == want.tobytes()
        assert got_t.is_cuda and got_t.dtype == torch.int32 and got_t.shape == torch.Size(want.shape) and got_t.cpu().numpy().tobytes() == want.tobytes()

    want, exact = W.watershed(A, M, G, connectivity=2)
    both(dict(connectivity=2, return_stats=True), (A, M, G), want, exact)
    both(dict(connectivity=2), (A, M.astype(np.int64), G.astype(np.uint8) * 9), want)
    both(dict(direction="falling"), (A, M), W.watershed(A, M, direction="falling")[0])
    # no markers: the labelled regional minima (rising) or maxima (falling) at the same connectivity
    for direction, method, connectivity in (("rising", "erosion", 1), ("falling", "dilation", 3)):
        X = recon_ref.reconstruct(A, "step", method=method, connectivity=connectivity, out_kind="changed")[0]
        markers, k = label_ref.label(X, 0.5, "high", connectivity)
        assert k > 3
        want = W.watershed(A, markers, None, connectivity=connectivity, direction=direction)[0]
        both(dict(direction=direction, connectivity=connectivity), (A,), want)
        assert want.min() >= 1
    # float64 goes through float32, bool counts as uint8; two dimensions and one
    D = rng.randint(-4, 5, size=(23, 70)) * 0.25
    M2 = three_labels((1, 23, 70), 43).reshape(23, 70)
    both({}, (D, M2), W.watershed(R.pad3(D.astype(np.float32)), R.pad3(M2))[0].reshape(D.shape))
    both({}, (D[3], M2[3] + M2[5]), W.watershed(R.pad3(D[3].astype(np.float32)), R.pad3(M2[3] + M2[5]))[0].reshape(-1))
    Bm = rng.uniform(size=(23, 70)) < 0.5
    both(dict(direction="falling"), (Bm, M2), W.watershed(R.pad3(Bm.view(np.uint8)), R.pad3(M2), direction="falling")[0].reshape(Bm.shape))


def test_volume_argument_checks_on_the_device():
    import torch
    from contourist_amd import volume
    A = np.zeros((3, 4, 5), dtype=np.float32)
    M = np.zeros((3, 4, 5), dtype=np.int32)
    with pytest.raises(AssertionError):
        volume.watershed(torch.from_numpy(A).cuda(), M)      # markers beside the relief
    with pytest.raises(AssertionError):
        volume.watershed(A, torch.from_numpy(M).cuda())
