"""the regions calls (csrc/cx_regions.hip: cx_grid_regions3d, _select, _map, _contacts) against their numpy restatement
(tests/regions_ref.py): every field of every record exactly, the float vsum within the bound of a sum in any order; shapes around the
tile of 64 columns, label patterns that reach the group path, the per-lane path and the carried majority, every sample type from the
host and from the device, cropped masks, maps, contacts through an overflowing table, the march per label end to end, what a call
leaves alone, the error codes, and contourist_amd.volume."""
import numpy as np
import pytest

import regions_ref as R

pytestmark = pytest.mark.gpu

_cache = {}


def labels_of(shape, kind):
    key = (shape, kind)
    if key not in _cache:
        _cache[key] = R.pattern(shape, kind)
        _cache[key].setflags(write=False)
    return _cache[key]


def ref_of(what, shape, kind):
    key = (what, shape, kind)
    if key not in _cache:
        _cache[key] = {"regions": R.regions, "contacts": R.contacts}[what](labels_of(shape, kind))
    return _cache[key]


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def on_device(a):
    "a numpy array as a device tensor of the same bytes (uint16, which torch does not copy, as int16)"
    import torch
    a = np.array(a, order="C")      # (a copy: the cached patterns are read-only)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    torch.cuda.synchronize()
    return t


def peek(ptr, shape, dtype):
    "the bytes of a buffer of the context's, read without any call of the context"
    import torch
    from contourist_amd import volume
    return volume._device_view(ptr, shape, np.dtype(dtype).str, torch.device("cuda", 0)).cpu().numpy().tobytes()


def same_records(got, want, float_values=False, abs_sum=None):
    from contourist_amd import _ffi
    assert got.dtype == _ffi.REGION_DTYPE == R.REGION_DTYPE and len(got) == len(want)
    for name in R.REGION_DTYPE.names:
        if name == "vsum" and float_values:
            continue
        assert got[name].tobytes() == want[name].tobytes(), name      # bytes: -0.0 is not +0.0
    if float_values:
        g, w = got["vsum"], want["vsum"]
        exact = ~np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[exact & ~np.isnan(w)], w[exact & ~np.isnan(w)])
        err, bound = np.abs(g[~exact] - w[~exact]), R.vsum_bound(want, abs_sum)[~exact]
        print("worst |vsum - fsum| / bound:", float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
        assert np.all(err <= bound)


# ---- records ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.PATTERNS)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_records_and_contacts_of_every_shape_and_pattern(ctx, shape, kind):
    L = labels_of(shape, kind)
    device = (sum(shape) + len(kind)) % 2 == 1
    t = on_device(L) if device else None
    arg = (t.data_ptr(), shape) if device else L
    want = ref_of("regions", shape, kind)
    assert ctx.regions_grid(arg, count_only=True) == (len(want), int((L < 0).sum()))
    same_records(ctx.regions_grid(arg), want)
    pairs = ref_of("contacts", shape, kind)
    got = ctx.regions_contacts(arg)
    assert got.dtype == R.CONTACT_DTYPE and got.tobytes() == pairs.tobytes()
    assert ctx.regions_contacts(arg).tobytes() == got.tobytes()      # a second call: the same bytes


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", R.DTYPE_NAMES)
def test_values_of_every_sample_type(ctx, name, device):
    for shape, kind in (((2, 6, 65), "voronoi5"), (R.STRADDLE, "voronoi200_zero"), ((3, 5, 64), "noise")):
        L = labels_of(shape, kind)
        V, _ = R.typed_values(shape, name)
        want, abs_sum = R.regions(L, V, name, with_abs=True)
        if device:
            tv = on_device(V)
            values = (tv.data_ptr(), name, shape)
        else:
            values = (V, name, shape)
        got = ctx.regions_grid(L, values)
        same_records(got, want, name in R.FLOAT_NAMES, abs_sum)
        if name in R.FLOAT_NAMES:
            assert got["n_nan"].sum() > 0 and np.all(got["isum"] == 0)
        else:
            assert np.array_equal(got["vsum"], got["isum"].astype(np.float64))


def test_float_sums_of_values_that_do_not_add_exactly(ctx):
    rng = np.random.RandomState(3)
    for kind in ("voronoi5", "noise", "one"):
        L = labels_of(R.STRADDLE, kind)
        V = (rng.standard_normal(R.STRADDLE) * 1e3).astype(np.float32)
        want, abs_sum = R.regions(L, V, with_abs=True)
        same_records(ctx.regions_grid(L, V), want, True, abs_sum)


@pytest.mark.parametrize("name", R.FLOAT_NAMES)
def test_minus_zero_is_below_plus_zero_and_a_region_of_nans(ctx, name):
    shape = (2, 3, 131)
    L = np.ones(shape, dtype=np.int32)
    L[1] = 2
    V = R.zeros_only(shape, name)
    got = ctx.regions_grid(L, (V, name, shape))
    same_records(got, R.regions(L, V, name, with_abs=True)[0], True, np.zeros(2))
    # (-0.0 sits at the odd indices; the second region starts at the odd index 393)
    assert list(got["min_at"]) == [1, 393] and list(got["max_at"]) == [0, 394] and np.all(np.signbit(got["vmin"])) and not np.any(np.signbit(got["vmax"]))
    nan = {"float32": np.float32(np.nan), "float16": np.float16(np.nan), "bfloat16": np.uint16(0x7FC0)}[name]
    V = V.copy()
    V[1] = nan
    got = ctx.regions_grid(L, (V, name, shape))
    same_records(got, R.regions(L, V, name, with_abs=True)[0], True, np.zeros(2))
    assert got["n_nan"][1] == 3 * 131 and got["min_at"][1] == got["max_at"][1] == -1 and got["vmin"][1] == got["vmax"][1] == got["vsum"][1] == 0


def test_the_largest_label_served_and_the_one_above_refused():
    from contourist_amd import _ffi
    c = _ffi.Context()
    try:
        L = np.zeros((1, 2, 3), dtype=np.int32)
        L[0, 1, 1] = _ffi.CX_REGIONS_MAX_LABEL
        L[0, 0, 2] = 5
        got = c.regions_grid(L, np.full(L.shape, 9, dtype=np.uint8))
        assert len(got) == _ffi.CX_REGIONS_MAX_LABEL == R.MAX_LABEL and got["voxels"].sum() == 2
        assert got[-1]["first"] == 4 and got[-1]["isum"] == 9 and got[4]["first"] == 2 and got[7]["first"] == -1 and got[7]["hi"][2] == -1
        L[0, 0, 0] = _ffi.CX_REGIONS_MAX_LABEL + 1
        for call in (lambda: c.regions_grid(L), lambda: c.regions_grid(L, count_only=True)):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_UNSUPPORTED
    finally:
        c.close()


def test_labels_by_the_result_pointers_of_watershed_and_label(ctx):
    import label_ref
    import watershed_ref
    rng = np.random.RandomState(8)
    shape = (9, 10, 70)
    A = (rng.standard_normal(shape) * 3.0).astype(np.float32)
    k, lptr = ctx.label_grid(0.5, "high", 1, samples=A)
    labels, k_ref = label_ref.label(A, 0.5, "high", 1)
    assert k == k_ref and ctx.label_result()[1] == lptr
    same_records(ctx.regions_grid((lptr, shape), A), R.regions(labels, A, with_abs=True)[0], True, R.regions(labels, A, with_abs=True)[1])
    assert ctx.regions_grid((lptr, shape))["voxels"].tobytes() == ctx.label_measures()["voxels"].tobytes()
    M = np.where(rng.uniform(size=shape) < 0.01, rng.randint(1, 30, size=shape), 0).astype(np.int32)
    _, wptr = ctx.watershed_grid(M, samples=A)
    flooded = watershed_ref.watershed(A, M)[0]
    same_records(ctx.regions_grid((wptr, shape)), R.regions(flooded))
    assert ctx.regions_contacts((wptr, shape)).tobytes() == R.contacts(flooded).tobytes()
    assert ctx.watershed_result() == (shape, wptr) and ctx.label_result()[1] == lptr      # read where they lie, and left there


# ---- select ----------------------------------------------------------------------------------------------------------------------------
def test_select_whole_boxes_pads_corners_and_short_keeps(ctx):
    L = labels_of(R.STRADDLE, "voronoi200_zero")
    rec = ref_of("regions", R.STRADDLE, "voronoi200_zero")
    t = on_device(L)
    c = int(np.argmax(rec["voxels"])) + 1
    keep_one = np.zeros(c + 1, dtype=np.uint8)      # shorter than K + 1
    keep_one[c] = 1
    keep_many = (np.arange(len(rec) + 1) % 3 == 1).astype(np.uint8)
    keep_back = np.array([1, 0, 1], dtype=np.uint8)      # the background and label 2
    far = tuple(n - 1 for n in R.STRADDLE)
    own = (tuple(rec["lo"][c - 1]), tuple(rec["hi"][c - 1]))
    cases = [(keep_many, None, 0), (keep_back, None, 1), (keep_one, own, 0), (keep_one, own, 1), (keep_one, own, 8),
             (keep_many, ((0, 0, 0), (3, 2, 5)), 8), (keep_many, ((far[0] - 2, far[1] - 1, far[2] - 70), far), 8), (keep_many, ((0, 0, 0), far), 3),
             (keep_many, ((5, 6, 7), (5, 6, 7)), 0), (keep_many, ((5, 6, 7), (5, 6, 7)), 2), (keep_many, (far, far), 8), (np.zeros(0, np.uint8), None, 0)]
    for n, (keep, box, pad) in enumerate(cases):
        want, origin, ones = R.select_fast(L, keep, box, pad)
        arg = (t.data_ptr(), R.STRADDLE) if n % 2 else L
        got_ones, shape, got_origin, got = ctx.regions_select(arg, keep, box, pad, download=True)
        assert (got_ones, shape, got_origin) == (ones, want.shape, origin) and got.tobytes() == want.tobytes(), (n, box, pad)
        assert ctx.regions_mask_result() == (want.shape, ctx.regions_mask_result()[1], origin, ones)
    assert ones == 0 and R.select_fast(L, keep_one, own, 0)[2] == rec["voxels"][c - 1]


def test_select_into_misaligned_outputs_between_guard_bytes(ctx):
    import torch
    L = labels_of((3, 5, 63), "voronoi5")
    keep = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint8)
    for pad, box in ((0, None), (2, ((1, 1, 3), (2, 4, 40)))):
        want, origin, ones = R.select_fast(L, keep, box, pad)
        for shift in (0, 1, 7, 15, 16, 17):
            room = torch.full((want.size + 96,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            at = room.data_ptr() + 32 + shift
            got_ones, shape, got_origin, ptr = ctx.regions_select(L, keep, box, pad, out=at)
            assert (got_ones, shape, got_origin, ptr) == (ones, want.shape, origin, at)
            back = room.cpu().numpy()
            assert back[32 + shift:32 + shift + want.size].tobytes() == want.tobytes()
            assert np.all(back[:32 + shift] == 0xAB) and np.all(back[32 + shift + want.size:] == 0xAB)
    from contourist_amd import _ffi
    with pytest.raises(_ffi.CxError) as e:      # a caller's output leaves nothing pending
        ctx.regions_mask_result()
    assert e.value.code == _ffi.CX_ERR_STATE


# ---- map -------------------------------------------------------------------------------------------------------------------------------
def test_map_identity_sequential_merge_short_table_and_in_place(ctx):
    import torch
    for shape in ((2, 3, 131), (1, 1, 1), (5, 4, 3)):
        L = labels_of(shape, "gaps")
        k = int(L.max())
        identity = np.arange(k + 1, dtype=np.int32)
        assert ctx.regions_map(L, identity, download=True).tobytes() == L.tobytes()
        present = np.unique(L[L > 0])
        forward = np.zeros(k + 1, dtype=np.int32)
        forward[present] = np.arange(1, len(present) + 1)
        got = ctx.regions_map(L, forward, download=True)
        assert got.tobytes() == R.relabel(L, forward).tobytes() and set(np.unique(got)) == set(range(1, len(present) + 1))
        merge = identity.copy()
        merge[14] = 7
        merge[0] = -2      # the background can be given a value too
        assert ctx.regions_map(L, merge, download=True).tobytes() == R.relabel(L, merge).tobytes()
        short = identity[:15]
        assert ctx.regions_map(L, short, download=True).tobytes() == R.relabel(L, short).tobytes() and (R.relabel(L, short) == 0).any() == (k > 14)
        # on the device: into a caller's buffer at an odd int32 offset, then in place
        room = torch.zeros(L.size + 9, dtype=torch.int32, device="cuda")
        t = on_device(L)
        out = room.data_ptr() + 12
        assert ctx.regions_map((t.data_ptr(), shape), merge, out=out) == out
        back = room.cpu().numpy()
        assert back[3:3 + L.size].tobytes() == R.relabel(L, merge).tobytes() and not back[:3].any() and not back[3 + L.size:].any()
        assert np.array_equal(t.cpu().numpy(), L)
        ctx.regions_map((t.data_ptr(), shape), merge, out=t.data_ptr())
        assert t.cpu().numpy().tobytes() == R.relabel(L, merge).tobytes()
        assert ctx.regions_map((t.data_ptr(), shape), np.zeros(0, np.int32), download=True).tobytes() == np.zeros(shape, np.int32).tobytes()
    negative = labels_of((5, 4, 3), "negative")
    table = np.array([9, 1, 2, 3, 4, 5], dtype=np.int32)
    assert ctx.regions_map(negative, table, download=True).tobytes() == R.relabel(negative, table).tobytes()


# ---- contacts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["voronoi200", "noise"])
def test_contacts_through_a_table_that_overflows(kind):
    from contourist_amd import _ffi
    L = labels_of(R.STRADDLE, kind)
    want = ref_of("contacts", R.STRADDLE, kind)
    assert len(want) > R.TABLE_MIN_PAIRS
    c = _ffi.Context()
    try:
        before = _ffi.device_bytes(c.handle)
        got = c.regions_contacts(L)      # the first call of a fresh context: a table of 1024 slots, doubled until the pairs fill at most half
        held, allocations = _ffi.device_bytes(c.handle)
        assert got.tobytes() == want.tobytes()
        doublings = int(np.ceil(np.log2(2 * len(want) / 1024.0)))
        assert doublings >= 1 and held - before[0] >= 32 * 1024 * 2 ** doublings and allocations - before[1] >= 1 + doublings
        assert c.regions_contacts(L).tobytes() == want.tobytes()
        assert _ffi.device_bytes(c.handle) == (held, allocations)      # the table is kept: the second call runs once and allocates nothing
    finally:
        c.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def test_two_balls_split_measured_and_marched_per_label():
    import distance_ref
    from contourist_amd import _ffi, volume
    shape = (48, 48, 48)
    centres = ((24, 24, 16), (24, 24, 32))
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).astype(np.float64)
    inside = np.zeros(shape, dtype=bool)
    for centre in centres:
        inside |= ((g - np.array(centre)) ** 2).sum(-1) <= 11.0 ** 2
    A = inside.astype(np.float32)
    labels = volume.split_touching(A, 0.5, 1.0)
    D = distance_ref.distance(A, 0.5, "above").astype(np.float32)
    rec = volume.regions(labels, D)
    want, abs_sum = R.regions(labels, D, with_abs=True)
    same_records(rec, want, True, abs_sum)
    assert len(rec) == 2 and np.all(rec["voxels"] > 0) and rec["voxels"].sum() == inside.sum()
    for c in range(2):
        peak = np.unravel_index(int(rec["max_at"][c]), shape)
        assert max(abs(int(p) - q) for p, q in zip(peak, centres[c])) <= 1, (peak, centres[c])
    pairs = volume.contacts(labels)
    both = pairs[(pairs["a"] == 1) & (pairs["b"] == 2)]
    assert len(both) == 1 and both["faces"].sum() > 0 and both["faces"][0][2] > 0
    assert pairs.tobytes() == R.contacts(labels).tobytes()
    with_area = volume.contacts(labels, sampling=(2.0, 3.0, 5.0))
    assert np.array_equal(with_area["area"], pairs["faces"][:, 0] * 15.0 + pairs["faces"][:, 1] * 10.0 + pairs["faces"][:, 2] * 6.0)
    whole = _ffi.Context()
    try:
        seen = []
        for c, points, triangles in volume.region_surfaces(labels, pad=1):
            table = volume._context().level1_components()
            assert len(table) >= 1 and np.all(table["closed"] != 0)
            lo, hi = rec["lo"][c - 1].astype(np.float64), rec["hi"][c - 1].astype(np.float64)
            assert len(points) and np.all(points >= lo - 1) and np.all(points <= hi + 1)
            # the same label selected on the whole volume, bound and marched
            whole.regions_select(labels, np.arange(3) == c)
            whole.bind_region_mask()
            post = whole.postprocess3d() if whole.extract3d(0.5)["n_triangles"] else None
            wp, wt = whole.download_level1(post)
            assert len(wt) == len(triangles) and len(wp) == len(points)
            order = lambda p: p[np.lexsort(p.T[::-1])]
            assert np.array_equal(order(points), order(wp))
            scaled = next(volume.region_surfaces(labels, ids=[c], mins=(1.0, -2.0, 0.5), delta=(0.5, 2.0, 4.0)))[1]
            assert np.array_equal(order(scaled), order(wp * np.array([0.5, 2.0, 4.0]) + np.array([1.0, -2.0, 0.5])))
            seen.append(c)
        assert seen == [1, 2]
    finally:
        whole.close()


# ---- state -----------------------------------------------------------------------------------------------------------------------------
def test_what_a_call_leaves_alone_and_what_the_bind_resets():
    from contourist_amd import _ffi
    rng = np.random.RandomState(19)
    shape = (12, 13, 70)
    A = (rng.standard_normal(shape) * 3.0).astype(np.float32)
    L = R.pattern(shape, "voronoi5_zero")
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)      # the seven pending results (label: the labels and the mask)
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        c.label_select(np.arange(k + 1) % 2)
        mask = c.label_mask_result()
        c.resample_grid(np.diag([1.0, 0.5, 1.0]), np.zeros(3), shape)
        res = c.resample_result()
        _, qptr = c.rank_grid(3, 13)
        _, rptr = c.reconstruct_grid("shift", h=2.5, connectivity=2)
        _, wptr = c.watershed_grid(lptr)
        buffers = ((filt[1], filt[0], "float32"), (dist[1], shape, "float32"), (lptr, shape, "int32"), (mask[1], shape, "uint8"), (res[1], shape, "float32"),
                   (qptr, shape, "float32"), (rptr, shape, "float32"), (wptr, shape, "int32"))
        held = [peek(*b) for b in buffers]
        # the four calls, from the host, from the device, on the pending labels, and a pending mask of their own
        c.regions_grid(L, A)
        c.regions_grid((wptr, shape), (dist[1], "float32", shape))
        c.regions_contacts((lptr, shape))
        c.regions_map(L, np.arange(9), download=True)
        ones, mshape, origin, mptr = c.regions_select((wptr, shape), np.ones(k + 1), ((1, 2, 3), (4, 5, 60)), 2)
        assert c.regions_mask_result() == (mshape, mptr, origin, ones) and mshape == (8, 8, 62) and origin == (-1, 0, 1)
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts      # the grid is the one uploaded
        assert (c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (shape, lptr, "high", 2, k) and c.label_mask_result() == mask
                and c.resample_result() == res and c.rank_result() == (shape, qptr, "float32") and c.reconstruct_result() == (shape, rptr, "float32", "values")
                and c.watershed_result() == (shape, wptr))
        assert held == [peek(*b) for b in buffers]
        # the pending mask is a legal `samples` of the other operations
        flooded = np.frombuffer(held[-1], dtype=np.int32).reshape(shape)
        want = R.select_fast(flooded, np.ones(k + 1), ((1, 2, 3), (4, 5, 60)), 2)[0]
        assert peek(mptr, mshape, "uint8") == want.tobytes()
        assert c.rank_grid(1, 0, samples=(mptr, "uint8", mshape), download=True)[1].tobytes() == want.tobytes()
        # the bind: the mask is the grid, with every reset of an upload (the origin is the caller's, as across uploads); nothing is pending any more
        c.set_origin(*origin)
        c.bind_region_mask()
        assert c.grid_info() == dict(dtype="uint8", device_bytes=want.size) and c.shape == mshape
        with pytest.raises(_ffi.CxError) as e:      # the extraction and the Level-1 mesh of the grid before are gone
            c.counts()
        assert e.value.code == _ffi.CX_ERR_STATE
        fresh = _ffi.Context()
        try:
            fresh.set_origin(*origin)
            fresh.upload_grid_native(want)
            assert c.extract3d(0.5) == fresh.extract3d(0.5)
            assert all(np.array_equal(a, b) for a, b in zip(c.download_level0_records(c.counts()), fresh.download_level0_records(fresh.counts())))
        finally:
            fresh.close()
        with pytest.raises(_ffi.CxError) as e:
            c.regions_mask_result()
        assert e.value.code == _ffi.CX_ERR_STATE
        # a mask the march does not take stays pending
        c.regions_select(L, np.ones(9), ((0, 0, 0), (0, 5, 5)), 0)
        pending = c.regions_mask_result()
        with pytest.raises(_ffi.CxError) as e:
            c.bind_region_mask()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.regions_mask_result() == pending and c.grid_info()["dtype"] == "uint8"
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import torch
    from contourist_amd import _ffi
    fresh = _ffi.Context()
    try:
        for call in (fresh.regions_mask_result, fresh.bind_region_mask):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    shape = (4, 5, 6)
    L = labels_of(shape, "voronoi5")
    n = L.size
    big = torch.zeros(16 * n, dtype=torch.int32, device="cuda")
    l_in = big[4 * n:5 * n]
    l_in.copy_(torch.from_numpy(np.array(L).reshape(-1)))
    torch.cuda.synchronize()
    lib, h, lp = ctx.lib, ctx.handle, l_in.data_ptr()
    k, rec = ctypes_i64(), np.zeros(8, dtype=_ffi.REGION_DTYPE)
    lo, hi = np.zeros(3, dtype=np.int64), np.array([3, 4, 5], dtype=np.int64)
    keep, table = np.ones(6, dtype=np.uint8), np.arange(6, dtype=np.int32)
    out = big[8 * n:].data_ptr()

    def regions(labels=lp, shape=shape, values=None, dtype=0, capacity=8):
        return lib.cx_grid_regions3d(h, labels, 1, shape[0], shape[1], shape[2], values, dtype, 1, rec.ctypes.data, capacity, None, None)

    def select(labels=lp, shape=shape, n_keep=6, lo=lo, hi=hi, pad=0, out=out):
        return lib.cx_grid_regions3d_select(h, labels, 1, shape[0], shape[1], shape[2], keep.ctypes.data, n_keep, None if lo is None else lo.ctypes.data,
                                            None if hi is None else hi.ctypes.data, pad, out, None, None, None, None)

    def remap(labels=lp, shape=shape, n_map=6, out=out, host=None):
        return lib.cx_grid_regions3d_map(h, labels, 1, shape[0], shape[1], shape[2], table.ctypes.data, n_map, out, host)

    def pairs(labels=lp, shape=shape, capacity=64, room=np.zeros(64, dtype=_ffi.REGION_CONTACT_DTYPE)):
        return lib.cx_grid_regions3d_contacts(h, labels, 1, shape[0], shape[1], shape[2], room.ctypes.data, capacity, None)

    assert regions() == select() == remap() == pairs() == _ffi.CX_OK
    for call in (regions, select, remap, pairs):
        for bad in (dict(labels=None), dict(labels=lp + 2), dict(shape=(0, 5, 6)), dict(shape=(4, -1, 6)), dict(shape=(1 << 15, 1 << 14, 2)), dict(shape=(1 << 30, 1, 1))):
            assert call(**bad) == _ffi.CX_ERR_INVALID, (call.__name__, bad)
    assert lib.cx_grid_regions3d(None, lp, 1, 4, 5, 6, None, 0, 0, None, 0, None, None) == _ffi.CX_ERR_INVALID
    assert int(L.max()) > 1 and regions(capacity=int(L.max()) - 1) == _ffi.CX_ERR_INVALID and regions(values=lp, dtype=7) == _ffi.CX_ERR_INVALID and regions(values=lp, dtype=-1) == _ffi.CX_ERR_INVALID
    assert lib.cx_grid_regions3d(h, lp, 1, 4, 5, 6, None, 0, 0, None, 0, ctypes_ref(k), None) == _ffi.CX_OK and k.value == L.max()      # K alone
    assert pairs(capacity=1) == _ffi.CX_ERR_INVALID
    for bad in (dict(pad=-1), dict(pad=9), dict(lo=np.array([0, 0, -1], dtype=np.int64)), dict(hi=np.array([3, 5, 5], dtype=np.int64)),
                dict(lo=np.array([2, 0, 0], dtype=np.int64), hi=np.array([1, 4, 5], dtype=np.int64)), dict(lo=None), dict(hi=None), dict(n_keep=-1),
                dict(out=lp), dict(out=lp + 4 * n - 1), dict(out=lp - n + 1)):
        assert select(**bad) == _ffi.CX_ERR_INVALID, bad
    assert select(out=lp - n) == _ffi.CX_OK and select(out=lp + 4 * n) == _ffi.CX_OK      # next to the labels is fine
    l_in.copy_(torch.from_numpy(np.array(L).reshape(-1)))
    torch.cuda.synchronize()
    for bad in (dict(out=lp + 4), dict(out=lp - 4), dict(out=lp + 4 * n - 4), dict(out=out + 2), dict(out=None), dict(n_map=-1)):
        assert remap(**bad) == _ffi.CX_ERR_INVALID, bad
    assert remap(out=lp) == _ffi.CX_OK and remap(out=lp + 4 * n) == _ffi.CX_OK


def ctypes_i64():
    import ctypes
    return ctypes.c_int64()


def ctypes_ref(x):
    import ctypes
    return ctypes.addressof(x)


# ---- contourist_amd.volume ---------------------------------------------------------------------------------------------------------------
def test_volume_wrappers_numpy_tensors_and_fewer_dimensions():
    import torch
    from contourist_amd import volume
    rng = np.random.RandomState(4)
    for shape in ((70,), (9, 67), (4, 5, 66)):
        shape3 = (1,) * (3 - len(shape)) + shape
        L = (rng.randint(0, 6, size=shape) * 3).astype(np.int64)      # 0, 3, .. 15; any integer type
        V = rng.randint(-9, 9, size=shape).astype(np.int16)
        t, tv = torch.from_numpy(L).cuda(), torch.from_numpy(V).cuda()
        want = R.regions(L.reshape(shape3), V.reshape(shape3))
        for got in (volume.regions(L, V), volume.regions(t, tv), volume.regions(t, V)):
            same_records(got, want)
        same_records(volume.regions(L), R.regions(L.reshape(shape3)))
        # relabel: sequential by value; the forward map
        new, forward = volume.relabel(L)
        new_t, forward_t = volume.relabel(t)
        present = np.unique(L[L > 0])
        assert isinstance(new, np.ndarray) and new.dtype == np.int32 and new.shape == shape and new_t.is_cuda and new_t.dtype == torch.int32
        assert np.array_equal(forward, forward_t) and np.array_equal(new, new_t.cpu().numpy()) and np.array_equal(forward[present], np.arange(1, len(present) + 1))
        assert np.array_equal(new, forward[L]) and forward.sum() == forward[present].sum()
        # keep_regions: ids kept, the others 0
        sizes = want["voxels"]
        floor = int(np.median(sizes[sizes > 0]))
        kept = volume.keep_regions(L, min_voxels=floor)
        ok = np.concatenate([[False], sizes >= floor])
        assert np.array_equal(kept, np.where(ok[L], L, 0)) and np.array_equal(volume.keep_regions(t, min_voxels=floor).cpu().numpy(), kept)
        inner = volume.keep_regions(L, rim=False, keep=lambda records: records["voxels"] > 0)
        assert inner.shape == shape and not inner[(0,) * len(shape)] and not inner[tuple(n - 1 for n in shape)]
        # contacts and masks
        assert volume.contacts(L).tobytes() == R.contacts(L.reshape(shape3)).tobytes() == volume.contacts(t).tobytes()
        lo, hi = [1] * len(shape), [n - 2 for n in shape]
        lo3, hi3 = [0] * (3 - len(shape)) + lo, [0] * (3 - len(shape)) + hi
        for pad in (0, 2):
            mask, origin = volume.region_mask(L, [3, 9], (lo, hi), pad)
            ref = R.select_fast(L.reshape(shape3), np.isin(np.arange(10), (3, 9)), (lo3, hi3), pad)[0]
            for _ in range(3 - len(shape)):
                ref = ref[pad]
            mask_t, origin_t = volume.region_mask(t, [3, 9], (lo, hi), pad)
            assert origin == origin_t == tuple(x - pad for x in lo) and mask.shape == ref.shape and np.array_equal(mask, ref)
            assert mask_t.is_cuda and np.array_equal(mask_t.cpu().numpy(), ref)
        whole, origin = volume.region_mask(L, [0])
        assert origin == (0,) * len(shape) and np.array_equal(whole, (L == 0).astype(np.uint8))
