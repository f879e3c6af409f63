"""GPU: the growable device buffers of a context (cx_buf, cx_ctx.h) through the allocation counter cx_device_bytes.

Every family of calls runs small -> large -> small on ONE context and must give, download for download and bit for bit, what a fresh
context gives for the same input; a second identical call allocates nothing; after cx_ctx_destroy the process holds what it held
before cx_ctx_create; and live_bytes is the sum of the documented sizes.

The workgroups of the generic 3-D kernels and of the 4-D march reserve their output ranges with atomics, so the ORDER of their records
differs from run to run, between two fresh contexts as well, and everything downstream of the 4-D march inherits that order.  Those
downloads are compared in canonical form, every value still bit for bit: Level 0 with vertices sorted by edge id and cells as sorted
rows of edge ids (oracle.level0.canonical_level0 / oracle.level0_4d.canonical4, the equality every other test of those marches
uses), the 4-D post-pass, morph and slab meshes as sorted points and sorted rows of the cells' corner coordinates (_canon_mesh).
Everything else is compared as raw bytes."""
import gc
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

G4 = os.path.join(ROOT, "tests", "golden4d")
G2 = os.path.join(ROOT, "tests", "golden2d")
SHAPES3 = {"small": (29, 23, 67), "mid": (37, 41, 52), "large": (64, 64, 64)}   # those of test_exact_capacities
VALUE3 = 0.1


def _field3(size):
    shape = SHAPES3[size]
    rng = np.random.RandomState(11)
    g0, g1, g2 = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (np.sin(3.1 * g0 + 0.4) * np.cos(2.7 * g1) + 0.8 * np.sin(3.9 * g2 + 1.0) + 0.05 * rng.standard_normal(shape)).astype(np.float32)


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


def _families():
    from contourist_amd import _ffi
    return {"staged": _extract3d(_ffi.CX_DIAG_CPYTHON310), "generic": _extract3d(_ffi.CX_DIAG_CPYTHON310 | _ffi.CX_KERNEL_GENERIC),
            "levels": _levels, "seeded": _seeded, "level1": _level1, "level4": _level4, "slabs": _slabs, "contour2": _contour2}


FAMILIES = ["staged", "generic", "levels", "seeded", "level1", "level4", "slabs", "contour2"]
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
    "small, large, small again on one context: every download equals a fresh context's at the same input"
    from contourist_amd import _ffi
    run = _families()[name]
    ctx = _ffi.Context(0)
    try:
        for size in ("small", "large", "mid", "small"):
            _assert_same(run(ctx, size), _reference(name, size), "%s/%s" % (name, size))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_steady_state_allocates_nothing(name):
    "the second identical call finds every buffer large enough (what keeps allocations out of a timed loop)"
    from contourist_amd import _ffi
    run = _families()[name]
    ctx = _ffi.Context(0)
    try:
        first = run(ctx, "large")
        live, allocations = _ffi.device_bytes(ctx.handle)
        assert live > 0 and allocations > 0
        second = run(ctx, "large")
        print(name, "live bytes", live, "allocations", allocations, "after the second call", _ffi.device_bytes(ctx.handle))
        assert _ffi.device_bytes(ctx.handle) == (live, allocations)
        _assert_same(second, first, name)
    finally:
        ctx.close()


def test_nothing_is_left_behind():
    "every family on one context, destroyed with a level selected; another destroyed with a slab assembly open: the process is back at its start"
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
