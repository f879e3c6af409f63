"""GPU: the growable device buffers of a context (cx_buf, cx_ctx.h) through the allocation counter cx_device_bytes.

Every family of calls runs small -> large -> small on ONE context and must give, download for download and bit for bit, what a fresh
context gives for the same input; a second identical call allocates nothing; after cx_ctx_destroy the process holds what it held
before cx_ctx_create; and live_bytes is the sum of the documented sizes.  All families also run interleaved on one context, in three
orders; each whole-volume operation is fed its own pending result four times (test_chain).  A subsystem with state of its own has a
family here: a new one adds one.

The workgroups of the generic 3-D kernels and of the 4-D march reserve their output ranges with atomics, so the ORDER of their records
differs from run to run, between two fresh contexts as well, and everything downstream of the 4-D march inherits that order.  Those
downloads are compared in canonical form, every value still bit for bit: Level 0 with vertices sorted by edge id and cells as sorted
rows of edge ids (oracle.level0.canonical_level0 / oracle.level0_4d.canonical4, the equality every other test of those marches
uses), the 4-D post-pass, morph and slab meshes as sorted points and sorted rows of the cells' corner coordinates (_canon_mesh).
Everything else is compared as raw bytes.  That includes every download of the families that came after cx_buf, all of which march
with the staged kernels: the attributes, topology records and loops, clip meshes, normals and maps, the cap and its Level 1, the
selections and the spectrum, the typed grids' Level 0, the Level 1 of a caller's mesh and cx_surface_geometry's result, and the
results, labels, records, masks and counts of the six whole-volume operations (the header calls each of them reproducible bit for bit
in every call and context).  At size small those of the volume operations and the selections are compared with the numpy
restatements of tests/buffer_families.py as well."""
import gc
import os

import numpy as np
import pytest

import buffer_families as F
from buffer_families import SHAPES3, _field3
from conftest import ROOT

pytestmark = pytest.mark.gpu

G4 = os.path.join(ROOT, "tests", "golden4d")
G2 = os.path.join(ROOT, "tests", "golden2d")
VALUE3 = 0.1


def _field4(size):
    G = np.load(os.path.join(G4, {"small": "noise_9x8x10x8", "mid": "merge_11x11x11x9", "large": "test0_style_13x13x13x9"}[size] + ".npz"))
    return G["A"], float(G["value"])


def _field2(size):
    G = np.load(os.path.join(G2, {"small": "corner_9x8", "mid": "circle_24x20", "large": "noise_levels_48x37"}[size] + ".npz"))
    return G["A"], G["values"]


def _canon3(xyz, keys, tris):
    from oracle import level0
    return list(level0.canonical_level0(keys.astype(np.int64), xyz, tris.astype(np.int64)))


def _canon4(verts, keys, tets):
    from oracle import level0_4d
    return list(level0_4d.canonical4(keys.astype(np.int64), verts, tets.astype(np.int64)))


def _sorted_rows(a):
    a = np.ascontiguousarray(a)
    a = a.reshape(len(a), int(np.prod(a.shape[1:])))        # (also with no rows)
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def _canon_mesh(pts, *cells):
    """points as sorted rows; every cell array as sorted rows of its corners' coordinates, corner order kept (cells[k] indexes
    cells[k - 1], the first one the points: morph triangles -> segments -> points)"""
    out, corners = [_sorted_rows(pts)], pts
    for c in cells:
        corners = corners[c].reshape(len(c), c.shape[1] * corners.shape[1])
        out.append(_sorted_rows(corners))
    return out


# ---- the families: each runs its calls on `ctx` for the input of `size` and returns every download as a list of arrays --------------
def _extract3d(flags):
    def run(ctx, size):
        ctx.upload_grid(_field3(size))
        c = ctx.extract3d(VALUE3, flags)
        xyz, keys, tris = ctx.download_level0(c)
        ids, t, tris2 = ctx.download_level0_records(c)
        from contourist_amd import _ffi
        if flags & _ffi.CX_KERNEL_GENERIC:
            return _canon3(xyz, keys, tris) + _canon3(t[:, None], ids, tris2)
        return [xyz, keys, tris, ids, t, tris2]
    return run


def _levels(ctx, size):
    ctx.upload_grid(_field3(size))
    counts = ctx.extract3d_levels([-0.3, VALUE3, 0.5], 1)
    out = []
    for i in (2, 0, 1):
        ctx.select_level(i)
        out += list(ctx.download_level0(counts[i]))
    return out


def _seeded(ctx, size):
    A = _field3(size)
    ctx.upload_grid(A)
    c = ctx.extract3d(VALUE3, 1)
    _xyz, keys, _tris = ctx.download_level0(c)
    picks = np.sort(keys.astype(np.int64))[[0, len(keys) // 2]]
    lin, d = picks >> 3, picks & 7
    q = np.stack(np.unravel_index(lin, A.shape), axis=1)
    dv = np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1)
    got = ctx.select_seeded([[tuple(a), tuple(b)] for a, b in zip(q.tolist(), (q + dv).tolist())])
    tk, vk = ctx.seeded_masks(c)
    return [np.array([got["seed_voxels"], got["groups_kept"], got["triangles_kept"]]), tk, vk]


def _level1(ctx, size):
    ctx.upload_grid(_field3(size))
    ctx.extract3d(VALUE3, 1)
    post = ctx.postprocess3d(0)
    out = list(ctx.download_level1(post))
    out.append(ctx.level1_normals(post))
    table = ctx.level1_components()
    out.append(table)
    kept = ctx.level1_keep_components(np.arange(len(table)) % 2 == 0)
    out += list(ctx.download_level1(kept))
    simp = ctx.level1_simplify(2.0)
    out += list(ctx.download_level1(simp))
    out.append(ctx.level1_simplify_map(kept["n_vertices"]))
    return out


def _level4(ctx, size):
    A, v = _field4(size)
    ctx.set_origin4d(0, 0, 0, 0)
    ctx.upload_grid4d(A)
    c = ctx.extract4d(v, 1)
    out = _canon4(*ctx.download_level0_4d(c))
    post = ctx.postprocess4d(100)
    out += _canon_mesh(*ctx.download_level1_4d(post))
    pts, segs, tris, _n = ctx.morph_triangles()
    out += _canon_mesh(pts, segs, tris)
    for p, t in ctx.morph_eval_many(np.linspace(0.5, A.shape[3] - 1.5, 5)):
        out += _canon_mesh(p, t)
    return out


def _slabs(ctx, size, finish=True):
    A, v = _field4(size)
    cut = A.shape[0] // 2
    ctx.slab4d_begin(A.shape)
    ctx.set_origin4d(0, 0, 0, 0)
    ctx.upload_grid4d(np.ascontiguousarray(A[:cut + 1]))
    ctx.extract4d(v, 1)
    ctx.slab4d_append(0, cut)
    if not finish:
        return []
    ctx.set_origin4d(cut, 0, 0, 0)
    ctx.upload_grid4d(np.ascontiguousarray(A[cut:]))
    ctx.extract4d(v, 1)
    ctx.slab4d_append(cut, A.shape[0] - cut)
    post = ctx.slab4d_finish(100)
    ctx.set_origin4d(0, 0, 0, 0)
    return _canon_mesh(*ctx.download_level1_4d(post)) + [np.sort(ctx.slab4d_keys(post))]


def _contour2(ctx, size):
    A, values = _field2(size)
    pts, keys, chains, npairs = ctx.contour2d(A, values)
    return [pts, keys, chains, np.array([npairs])]


# ---- the subsystems that came after cx_buf.  Each binds its own grid first, so that it runs the same after any other family ------------
def _attributes(ctx, size):
    B = F.second_field(size)
    ctx.upload_grid(_field3(size))
    c = ctx.extract3d(VALUE3, 1)
    out = [ctx.level0_normals(c), ctx.level0_curvature(c), ctx.level0_sample(c, B)]
    post = ctx.postprocess3d(0)
    out += [ctx.level1_curvature(post), ctx.level1_sample(post, B)]
    assert c["n_vertices"] > 100 and post["n_vertices"] > 100
    assert all(len(a) and np.isfinite(a).all() and len(np.unique(a)) > 16 for a in out)
    return out


def _topology(ctx, size):
    ctx.upload_grid(_field3(size))
    ctx.extract3d(VALUE3, 1)
    post = ctx.postprocess3d(0)
    table = ctx.level1_topology()
    loops, verts = ctx.level1_boundary_loops()
    assert len(table) == post["n_components"] >= 1 and int(table["triangles"].sum()) == post["n_triangles"]
    assert len(loops) >= 1 and len(verts) == int(loops["count"].sum()) > 0      # the surface crosses the array's rim
    return [table, loops, verts]


def _clip(ctx, size):
    from contourist_amd import _ffi
    shape = SHAPES3[size]
    ctx.upload_grid(_field3(size))
    ctx.extract3d(VALUE3, 1)
    post = ctx.postprocess3d(0)
    cut = ctx.level1_clip_plane((0.2, 0.1, 1.0), 0.45 * shape[2] + 0.2 * 0.5 * shape[0], _ffi.CX_CLIP_NORMALS)
    info = ctx.level1_clip_info()
    # a cut triangle hands at most two to the tail, a triangle kept whole one; some are dropped
    assert cut["n_cut_triangles"] > 0 and cut["n_raw_triangles"] > 2 * cut["n_cut_triangles"] and cut["n_raw_triangles"] < post["n_triangles"]
    assert info["n_triangles_before"] == post["n_triangles"] and info["cut_corners"] > 0
    out = list(ctx.download_level1(cut)) + [ctx.level1_normals(cut)] + list(ctx.level1_clip_map())
    post = ctx.postprocess3d(0)
    by_field = ctx.level1_clip_field(F.second_field(size), 0.0)
    assert by_field["n_cut_triangles"] > 0 and by_field["n_raw_triangles"] > 2 * by_field["n_cut_triangles"] and by_field["n_raw_triangles"] < post["n_triangles"]
    out += list(ctx.download_level1(by_field)) + list(ctx.level1_clip_map())
    out.append(np.array([cut[k] for k in sorted(cut)] + [by_field[k] for k in sorted(by_field)], dtype=np.int64))
    return out


def _cap(ctx, size):
    ctx.upload_grid(_field3(size))
    ctx.extract3d(VALUE3, 1)
    counts = ctx.cap3d("all")
    keys, tris = ctx.download_cap(counts)
    info = ctx.cap_info()
    post = ctx.postprocess3d_capped(0)
    assert len(keys) > 0 and len(tris) > 0 and info["n_rim_records"] > 0 and info["n_rim_points"] > 0
    return [keys, tris, np.array([info[k] for k in ("n_rim_records", "table_slots", "n_rim_points")], dtype=np.int64)] + list(ctx.download_level1(post))


def _pick(ctx, size):
    "the extraction made before the selections is downloaded after them (tests/test_gpu_select.py::test_extraction_survives, here across growth)"
    from contourist_amd import _ffi
    A, other = _field3(size), F.pick_samples()
    ctx.upload_grid(A)
    c = ctx.extract3d(VALUE3, 1)
    of_grid, nan_grid = ctx.samples_select(F.pick_ranks(A.size))
    of_host, nan_host = ctx.samples_select(F.pick_ranks(other.size), samples=other)
    spectrum = ctx.level_spectrum3d(F.PICK_VALUES)
    assert nan_grid == 0 and nan_host == 0 and ctx.counts() == c
    assert spectrum["n_triangles"][F.PICK_VALUES.index(VALUE3)] == c["n_triangles"] > 0
    return [of_grid, of_host] + [spectrum[k] for k in _ffi.SPECTRUM_KEYS] + list(ctx.download_level0(c)) + list(ctx.download_level0_records(c))


def _typed(ctx, size):
    "one grid_owned under three sample types in turn"
    out = []
    for name in ("uint8", "int16", "float32"):
        Q = _field3(size) if name == "float32" else F.quantised(size, name)
        value = VALUE3 if name == "float32" else F.TYPED_VALUES[name]
        if name == "float32":
            ctx.upload_grid(Q)
        else:
            ctx.upload_grid_native(Q)
        assert ctx.grid_info() == dict(dtype=name, device_bytes=Q.size * Q.dtype.itemsize)
        c = ctx.extract3d(value, 1)
        assert c["n_triangles"] > 100
        out += list(ctx.download_level0(c)) + list(ctx.download_level0_records(c))
    return out


def _caller_mesh(ctx, size):
    from contourist_amd import _ffi
    shape = SHAPES3[size]
    ctx.upload_grid(_field3(size))
    c = ctx.extract3d(VALUE3, 1)
    keys, _t, tris = ctx.download_level0_records(c)
    pts = ctx.level0_points_f64(c)
    order = np.argsort(keys, kind="stable")          # cx_postprocess3d_mesh: vertices in ascending edge-id order
    inv = np.empty(len(order), dtype=np.int32)
    inv[order] = np.arange(len(order), dtype=np.int32)
    pts, tris = pts[order].copy(), inv[tris.reshape(-1, 3)].copy()
    post = ctx.postprocess3d_mesh(pts, tris, [n - 1 for n in shape], flags=_ffi.CX_MESH_OF_THE_MARCH)
    out = list(ctx.download_level1(post))
    assert post["n_triangles"] > 100
    out += list(ctx.surface_geometry(pts, tris, True))
    assert len(out[3]) > 100
    return out


def _march_bound(ctx, value):
    "the grid an operation's bind left: marched and downloaded"
    c = ctx.extract3d(value, 1)
    assert c["n_triangles"] > 100, c
    return list(ctx.download_level0(c)) + list(ctx.download_level0_records(c))


# Every family of a volume operation: its calls on host samples, downloaded, come first, in the order of buffer_families.EXPECTED (the
# largest result first, so that the slot settles with it); then the bound grid in and the result kept; the result described, bound,
# marched and downloaded.
def _filter(ctx, size):
    A = _field3(size)
    ctx.upload_grid(A)
    shape, got = ctx.filter_grid(F.FILTER_AXES, F.FILTER_MODE, samples=A, download=True)
    kept_shape, ptr = ctx.filter_grid(F.FILTER_AXES_BOUND, F.FILTER_MODE)
    assert ctx.filter_result() == (kept_shape, ptr) and kept_shape == shape == A.shape and ptr
    ctx.bind_filtered()
    assert ctx.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
    return [got] + _march_bound(ctx, VALUE3)


def _distance(ctx, size):
    A = _field3(size)
    ctx.upload_grid(A)
    sites, dist = ctx.distance_grid(F.DISTANCE_VALUE, "signed", "float32", samples=A, download=True)
    sites_b, mask = ctx.distance_grid(F.DISTANCE_VALUE, "below", "mask", radius2=F.DISTANCE_RADIUS2, samples=A, download=True)
    assert 0 < sites < A.size and 0 < sites_b < A.size and 0 < int(mask.sum()) < A.size
    kept_sites, ptr = ctx.distance_grid(F.DISTANCE_VALUE, "below", "float32")
    assert ctx.distance_result() == (A.shape, ptr, "float32", kept_sites) and ptr and kept_sites == sites_b
    ctx.bind_distance()
    assert ctx.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
    return [dist, mask, np.array([sites, sites_b])] + _march_bound(ctx, 1.5)


def _label(ctx, size):
    A = _field3(size)
    ctx.upload_grid(A)
    c_host, c_bound = F.LABEL_CONNECTIVITIES
    k, labels = ctx.label_grid(F.LABEL_VALUE, "high", c_host, samples=A, download=True)
    records = ctx.label_measures()
    n, mask = ctx.label_select(F.keep_pattern(k), download=True)
    assert k >= 2 and len(records) == k and 0 < n < A.size
    k2, lptr = ctx.label_grid(F.LABEL_VALUE, "high", c_bound)
    assert k2 >= 2 and ctx.label_result() == (A.shape, lptr, "high", c_bound, k2) and lptr
    records2 = ctx.label_measures()
    n2, mptr = ctx.label_select(F.keep_pattern(k2))
    assert ctx.label_mask_result() == (A.shape, mptr, n2) and mptr and 0 < n2 < A.size
    ctx.bind_label_mask()
    assert ctx.grid_info() == dict(dtype="uint8", device_bytes=A.size)
    assert ctx.label_result() == (A.shape, lptr, "high", c_bound, k2)      # the labels stay
    return [labels, records, mask, records2, np.array([k, n, k2, n2])] + _march_bound(ctx, 0.5)


def _resample(ctx, size):
    A, U = _field3(size), F.quantised(size, "uint8")
    M, off = F.RESAMPLE_ZOOM
    Mt, offt = F.resample_turn(A.shape)
    ctx.upload_grid(A)
    out1, linear = ctx.resample_grid(M, off, A.shape, 1, F.RESAMPLE_MODE, F.RESAMPLE_CVAL, samples=A, download=True)      # the table kernel
    out0, nearest = ctx.resample_grid(Mt, offt, A.shape, 0, F.RESAMPLE_MODE, 7, samples=U, download=True)                  # the general one
    assert 0 < out1 < A.size and 0 < out0 < A.size and nearest.dtype == np.uint8
    kept_out, ptr = ctx.resample_grid(Mt, offt, A.shape, 1, "nearest")
    assert ctx.resample_result() == (A.shape, ptr, "float32", kept_out) and ptr and kept_out == out0
    ctx.bind_resampled()
    assert ctx.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
    return [linear, nearest, np.array([out1, out0])] + _march_bound(ctx, VALUE3)


def _rank(ctx, size):
    A, Q = _field3(size), F.quantised(size, "int16")
    g, e = F.RANK_GENERAL, F.RANK_EXTREME
    ctx.upload_grid(A)
    _, median = ctx.rank_grid(g["size"], g["rank"], mode=g["mode"], samples=A, download=True)        # the general kernel
    _, maximum = ctx.rank_grid(e["size"], e["rank"], mode=e["mode"], samples=Q, download=True)       # the separable one
    assert maximum.dtype == np.int16 and (median != A).any() and (maximum != Q).any()
    shape, ptr = ctx.rank_grid((3, 5, 3), 22, mode="reflect")
    assert ctx.rank_result() == (A.shape, ptr, "float32") and ptr and shape == A.shape
    ctx.bind_ranked()
    assert ctx.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
    return [median, maximum] + _march_bound(ctx, VALUE3)


def _reconstruct(ctx, size):
    A, U = _field3(size), F.quantised(size, "uint8")
    ctx.upload_grid(A)
    s1, shifted = ctx.reconstruct_grid("shift", h=F.RECON_SHIFT_H, connectivity=F.RECON_CONNECTIVITY, samples=A, download=True)
    s2, stepped = ctx.reconstruct_grid("step", connectivity=F.RECON_CONNECTIVITY, samples=U, download=True)
    s3, marked = ctx.reconstruct_grid(F.recon_marker(size), connectivity=F.RECON_CONNECTIVITY, samples=A, download=True)      # a host marker: in2
    assert all(s["n_changed"] > 0 for s in (s1, s2, s3)) and s3["n_clamped"] > 0 and stepped.dtype == np.uint8
    s4, ptr = ctx.reconstruct_grid("shift", h=2 * F.RECON_SHIFT_H, connectivity=3)
    assert ctx.reconstruct_result() == (A.shape, ptr, "float32", "values") and ptr and s4["n_changed"] > 0
    ctx.bind_reconstructed()
    assert ctx.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
    counts = np.array([[s["n_changed"], s["n_clamped"]] for s in (s1, s2, s3, s4)])
    return [shifted, stepped, marked, counts] + _march_bound(ctx, VALUE3)


def _families():
    from contourist_amd import _ffi
    return {"staged": _extract3d(_ffi.CX_DIAG_CPYTHON310), "generic": _extract3d(_ffi.CX_DIAG_CPYTHON310 | _ffi.CX_KERNEL_GENERIC),
            "levels": _levels, "seeded": _seeded, "level1": _level1, "level4": _level4, "slabs": _slabs, "contour2": _contour2,
            "attributes": _attributes, "topology": _topology, "clip": _clip, "cap": _cap, "pick": _pick, "typed": _typed,
            "caller_mesh": _caller_mesh, "filter": _filter, "distance": _distance, "label": _label, "resample": _resample, "rank": _rank,
            "reconstruct": _reconstruct}


FAMILIES = ["staged", "generic", "levels", "seeded", "level1", "level4", "slabs", "contour2",
            "attributes", "topology", "clip", "cap", "pick", "typed", "caller_mesh", "filter", "distance", "label", "resample", "rank", "reconstruct"]
# A bind MOVES the slot's result into the context's grid and releases the grid owned before, so the next call of that
# operation makes its result buffer anew: one allocation in a second identical walk of a family that binds.  label's mask has a quarter
# of the bytes of the float32 grid uploaded after it, so there the upload regrows the grid too.
REBOUND_ALLOCATIONS = {"filter": 1, "distance": 1, "label": 2, "resample": 1, "rank": 1, "reconstruct": 1}
_fresh = {}


def _reference(name, size):
    "what a fresh context gives: computed once per (family, size), shared and never changed"
    from contourist_amd import _ffi
    if (name, size) not in _fresh:
        ctx = _ffi.Context(0)
        try:
            _fresh[(name, size)] = _families()[name](ctx, size)
        finally:
            ctx.close()
    return _fresh[(name, size)]


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), "%s: download %d differs from a fresh context's" % (what, i)


@pytest.mark.parametrize("name", FAMILIES)
def test_reuse_across_growth(name):
    """small, large, small again on one context: every download equals a fresh context's at the same input; and the step from small to
    large does allocate (a family whose buffers never regrow would not be testing growth)"""
    from contourist_amd import _ffi
    run = _families()[name]
    ctx = _ffi.Context(0)
    try:
        for size in ("small", "large", "mid", "small"):
            _, before = _ffi.device_bytes(ctx.handle)
            _assert_same(run(ctx, size), _reference(name, size), "%s/%s" % (name, size))
            _, after = _ffi.device_bytes(ctx.handle)
            print(name, size, "allocations", after - before)
            if size == "large":
                assert after > before, "%s: nothing regrew from small to large" % name
    finally:
        ctx.close()


@pytest.mark.parametrize("name", sorted(F.EXPECTED))
def test_small_is_what_the_restatement_gives(name):
    """the fresh context's downloads of the volume operations and the selections at size small, byte for byte against the numpy
    restatements (tests/buffer_families.py): what every other comparison of this file leans on is not only the code under test"""
    want, got = F.EXPECTED[name](), _reference(name, "small")
    assert 0 < len(want) <= len(got)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (name, i, a.shape, b.shape, a.dtype, b.dtype)
        assert a.tobytes() == b.tobytes(), "%s: download %d differs from the restatement" % (name, i)


def test_every_family_on_one_context():
    """all families on ONE context, three walks in three fixed orders at large, small, mid: scratch that two subsystems share (the
    Level-1 buffers of components, simplify, clip and topology), and what one leaves for the next (a bound grid replaced under a pending
    selection, a Level-1 mesh replaced under clip or topology tables, a typed grid before fp32 attributes, a pending result of another
    size in every slot)"""
    from contourist_amd import _ffi
    shuffled = [FAMILIES[i] for i in np.random.RandomState(5).permutation(len(FAMILIES))]
    ctx = _ffi.Context(0)
    try:
        for order, size in ((FAMILIES, "large"), (FAMILIES[::-1], "small"), (shuffled, "mid")):
            for name in order:
                _assert_same(_families()[name](ctx, size), _reference(name, size), "%s/%s after %s" % (name, size, order[max(0, order.index(name) - 1)]))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_steady_state_allocates_nothing(name):
    """the second identical call finds every buffer large enough (what keeps allocations out of a timed loop); a family that binds its
    result allocates exactly what the bind gave away (REBOUND_ALLOCATIONS), and holds no more bytes than before"""
    from contourist_amd import _ffi
    run = _families()[name]
    ctx = _ffi.Context(0)
    try:
        first = run(ctx, "large")
        live, allocations = _ffi.device_bytes(ctx.handle)
        assert live > 0 and allocations > 0
        second = run(ctx, "large")
        print(name, "live bytes", live, "allocations", allocations, "after the second call", _ffi.device_bytes(ctx.handle))
        assert _ffi.device_bytes(ctx.handle) == (live, allocations + REBOUND_ALLOCATIONS.get(name, 0))
        _assert_same(second, first, name)
    finally:
        ctx.close()


def test_nothing_is_left_behind():
    """every family on one context, destroyed with a level selected; another destroyed with a slab assembly open; a third with a pending
    result in every slot and a cap, a clip and topology tables resident: the process is back at its start"""
    from contourist_amd import _ffi
    gc.collect()      # contexts other tests dropped without close() go now, not in the middle of the count
    start, _ = _ffi.device_bytes(None)
    ctx = _ffi.Context(0)
    try:
        for name in FAMILIES:
            _families()[name](ctx, "mid")
        ctx.upload_grid(_field3("small"))
        ctx.extract3d_levels([-0.3, VALUE3, 0.5], 1)
        ctx.select_level(1)        # the context holds the level's output buffers, the level's slot the context's
        held, _ = _ffi.device_bytes(ctx.handle)
        assert held > 0 and _ffi.device_bytes(None)[0] == start + held
    finally:
        ctx.close()
    assert _ffi.device_bytes(None)[0] == start
    ctx = _ffi.Context(0)
    try:
        _slabs(ctx, "mid", finish=False)
        assert _ffi.device_bytes(None)[0] > start
    finally:
        ctx.close()
    assert _ffi.device_bytes(None)[0] == start
    # a third: closed while each of the six slots holds a pending result, label its labels and its mask, and a cap, a topology table and a clip are resident
    ctx = _ffi.Context(0)
    try:
        A = _field3("small")
        ctx.upload_grid(A)
        ctx.extract3d(VALUE3, 1)
        cap = ctx.cap3d("all")
        ctx.postprocess3d(0)
        assert len(ctx.level1_topology()) and len(ctx.level1_boundary_loops()[0])
        base, _ = _ffi.device_bytes(ctx.handle)
        clipped = ctx.level1_clip_plane((0.0, 0.0, 1.0), 0.5 * A.shape[2])
        assert clipped["n_cut_triangles"] > 0 and len(ctx.level1_clip_map()[0]) == clipped["n_vertices"] and len(ctx.level1_topology())
        ctx.filter_grid(F.FILTER_AXES, F.FILTER_MODE)
        ctx.distance_grid(F.DISTANCE_VALUE, "signed")
        k, _ = ctx.label_grid(F.LABEL_VALUE, "high", 1)
        ctx.label_select(F.keep_pattern(k))
        ctx.resample_grid(*F.RESAMPLE_ZOOM, out_shape=A.shape)
        ctx.rank_grid(3, 13)
        ctx.reconstruct_grid("shift", h=F.RECON_SHIFT_H)
        pending = (ctx.filter_result, ctx.distance_result, ctx.label_result, ctx.label_mask_result, ctx.resample_result, ctx.rank_result, ctx.reconstruct_result)
        assert all(result()[1] for result in pending) and len(ctx.download_cap(cap)[0])
        held, _ = _ffi.device_bytes(ctx.handle)
        # at least the clip's own and the results: three float32 volumes and one each of float32 distances, int32 labels and a uint8 mask
        assert held > base + (5 * 4 + 1) * A.size and _ffi.device_bytes(None)[0] == start + held
    finally:
        ctx.close()
    assert _ffi.device_bytes(None)[0] == start


def test_live_bytes_is_the_sum_of_the_capacities():
    """cx_reserve(c, v, t) holds 16 c + 8 v + 12 t bytes (16-byte cell records, 8-byte vertex records, three int32 per triangle); an
    uploaded grid its samples; the context itself its 2048 counter words"""
    from contourist_amd import _ffi
    A = _field3("large")
    ref = _ffi.Context(0)
    try:
        ref.upload_grid(A)
        counts = ref.extract3d(VALUE3, 1)
    finally:
        ref.close()
    c, v, t = counts["n_cells"], counts["n_vertices"], counts["n_triangles"]
    ctx = _ffi.Context(0)
    try:
        base, _ = _ffi.device_bytes(ctx.handle)
        assert _ffi.device_bytes(ctx.handle) == (2048 * 4, 1)
        ctx.reserve(c, v, t)
        assert _ffi.device_bytes(ctx.handle) == (base + 16 * c + 8 * v + 12 * t, 4)
        ctx.upload_grid(A)
        outputs_and_grid = base + 16 * c + 8 * v + 12 * t + A.size * 4
        assert _ffi.device_bytes(ctx.handle) == (outputs_and_grid, 5)
        assert ctx.extract3d(VALUE3, 1) == counts          # capacities equal to the counts: nothing regrows
        live, allocations = _ffi.device_bytes(ctx.handle)
        assert live >= outputs_and_grid and allocations > 5       # + the side tables of the staged kernels
        ctx.download_level0(counts)
        assert _ffi.device_bytes(ctx.handle)[0] == live + (v + v // 16 + 64) * 16      # the expanded float4 vertices, with their slack
    finally:
        ctx.close()


# ---- the chains: the pending result of call k is the samples of call k + 1, every result kept in the context (out=None) --------------
def _chain_call(ctx, op, samples, call):
    """call number `call` of the chain of `op` (buffer_families.chain_step, the same parameters) -> (its downloads, the pending result as
    the samples of the next call)"""
    if op == "filter":
        shape, got = ctx.filter_grid(F.FILTER_AXES, F.FILTER_MODE, samples=samples, download=True)
        described, ptr = ctx.filter_result()
        return [got], (ptr, "float32", described)
    if op == "distance":
        _, got = ctx.distance_grid(F.chain_distance_value(call), "signed", "float32", samples=samples, download=True)
        described, ptr, kind, _ = ctx.distance_result()
        return [got], (ptr, kind, described)
    if op == "label":
        k, labels = ctx.label_grid(F.chain_label_value(call), "high", F.LABEL_CONNECTIVITIES[0], samples=samples, download=True)
        assert k >= 2
        _, mask = ctx.label_select(F.chain_keep(k), download=True)
        described, ptr, _ = ctx.label_mask_result()
        return [labels, mask], (ptr, "uint8", described)
    if op == "resample":
        M, off = F.RESAMPLE_ZOOM
        shape = samples.shape if isinstance(samples, np.ndarray) else samples[2]
        n_outside, got = ctx.resample_grid(M, off, shape, 1, F.RESAMPLE_MODE, F.RESAMPLE_CVAL, samples=samples, download=True)
        assert n_outside > 0
        described, ptr, dtype, _ = ctx.resample_result()
        return [got], (ptr, dtype, described)
    if op == "rank":
        g = F.RANK_GENERAL
        _, got = ctx.rank_grid(g["size"], g["rank"], mode=g["mode"], samples=samples, download=True)
        described, ptr, dtype = ctx.rank_result()
        return [got], (ptr, dtype, described)
    assert op == "reconstruct"
    stats, got = ctx.reconstruct_grid("shift", h=F.RECON_SHIFT_H, connectivity=F.RECON_CONNECTIVITY, samples=samples, download=True)
    assert stats["n_changed"] > 0
    described, ptr, dtype, _ = ctx.reconstruct_result()
    return [got], (ptr, dtype, described)


def _on_a_fresh_context(op, host_samples, call):
    from contourist_amd import _ffi
    fresh = _ffi.Context(0)
    try:
        return _chain_call(fresh, op, host_samples, call)[0]
    finally:
        fresh.close()


# The allocations of a chain's second call.  The pending result steps aside into `in`, which the first call made for the
# host samples and which has room for the next result: filter, distance, resample and rank run on those two buffers from the start.
# Reconstruction keeps its host mask in `in` and steps aside into `prev`, which its second call creates.  Labelling reads the pending
# mask into the labels before the selection writes the mask again: one buffer, nothing steps aside.
CHAIN_SECOND_CALL_ALLOCATIONS = {"filter": 0, "distance": 0, "label": 0, "resample": 0, "rank": 0, "reconstruct": 1}


@pytest.mark.parametrize("size", ["small", "large"])
@pytest.mark.parametrize("op", F.OPERATIONS)
def test_chain(op, size):
    """four calls at one size, each on the pending result of the one before (label: on the pending mask of its selection): every download
    equals that of a fresh context given the previous download as host samples and, at size small, the restatement applied once more;
    the third and the fourth call allocate nothing (a chain settles on two buffers), the second what is documented above"""
    from contourist_amd import _ffi
    want = F.chain_expected(op) if size == "small" else None
    ctx = _ffi.Context(0)
    try:
        host, samples, tally = _field3(size), _field3(size), []
        for call in range(F.CHAIN_CALLS):
            got, samples = _chain_call(ctx, op, samples, call)
            tally.append(_ffi.device_bytes(ctx.handle))
            assert samples[0] and tuple(samples[2]) == SHAPES3[size]
            _assert_same(got, _on_a_fresh_context(op, host, call), "%s chain/%s call %d" % (op, size, call))
            if want:
                _assert_same(got, want[call], "%s chain call %d against the restatement" % (op, call))
            host = got[-1]
        print(op, size, "(live bytes, allocations) after each call", tally)
        assert tally[3] == tally[2], tally
        assert tally[1][1] - tally[0][1] == CHAIN_SECOND_CALL_ALLOCATIONS[op], tally
        if op == "reconstruct":      # the mask and the marker both lie in the pending result: planes 0 .. n - 2 and 1 .. n - 1 (F.inside_expected)
            ptr, dtype, shape = samples
            part, plane = (shape[0] - 1,) + tuple(shape[1:]), shape[1] * shape[2] * 4
            stats, got = ctx.reconstruct_grid((ptr + plane, dtype, part), method="erosion", connectivity=F.RECON_CONNECTIVITY, samples=(ptr, dtype, part),
                                              download=True)
            assert stats["n_changed"] > 0 and stats["n_clamped"] > 0 and _ffi.device_bytes(ctx.handle) == tally[3]
            assert ctx.reconstruct_result()[0] == part
            fresh = _ffi.Context(0)
            try:
                other = fresh.reconstruct_grid(np.ascontiguousarray(host[1:]), method="erosion", connectivity=F.RECON_CONNECTIVITY,
                                               samples=np.ascontiguousarray(host[:-1]), download=True)[1]
            finally:
                fresh.close()
            _assert_same([got], [other], "reconstruct chain/%s, the marker inside the mask's buffer" % size)
            if want:
                _assert_same([got], want[F.CHAIN_CALLS], "reconstruct chain, the marker inside the mask's buffer, against the restatement")
    finally:
        ctx.close()
