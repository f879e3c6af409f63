"""GPU: the default Level-0 step with 8-byte cell records between the vertex and the triangle stage (the {first triangle, first
vertex} of every 64th record beside them), full records rebuilt on demand for the seeded selection, one context taken through
shapes, paths and regrown capacities in turn (the chunk totals and every side table start clean each time), and the kernel
timing whose events are made when it is switched on."""
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6      # as tests/test_gpu_level0.py: vertex coordinates within 1e-6 relative fp32, with an absolute floor near 0
ABS_FLOOR = 1e-6


def _axes(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def _smooth(shape, seed, noise=0.05):
    rng = np.random.RandomState(seed)
    i, j, k = _axes(shape)
    A = np.sin(0.31 * i + 0.4) * np.cos(0.27 * j) + 0.8 * np.sin(0.19 * k + 1.0) + noise * rng.standard_normal(shape)
    return A.astype(np.float32)


def _tiny():
    i, j, k = _axes((9, 10, 12))
    return np.sqrt((i - 4.0) ** 2 + (j - 4.5) ** 2 + (k - 5.3) ** 2).astype(np.float32)


# name -> (samples, isovalue).  tiny: fewer than 64 records; odd: rows of 70 samples (the unaligned stream kernel) and a record count
# that is no multiple of 64; blocks: two k blocks of 256, three row blocks, several plane chunks -- the records of one group of 64 come
# from different streaming waves and batches; noise: nearly every cell active, most rounds full; ties: samples equal to the isovalue
# (the per-cell tolerance path writes the records)
FIELDS = {
    "tiny": lambda: (_tiny(), 1.3),
    "odd": lambda: (_smooth((33, 37, 70), 3), 0.1),
    "blocks": lambda: (_smooth((24, 40, 300), 4), 0.1),
    "noise": lambda: (np.random.RandomState(5).standard_normal((20, 20, 70)).astype(np.float32), 0.0),
    "ties": lambda: ((np.round(np.random.RandomState(6).standard_normal((12, 13, 14)) * 2) / 2).astype(np.float32), 0.5),
}
_fields = {}
_oracle = {}


def field(name):
    if name not in _fields:
        _fields[name] = FIELDS[name]()
    return _fields[name]


def oracle_mesh(name, value, diag_mode, origin):
    "the C oracle's Level-0 mesh, computed once per case: (march3d dict, edge ids, canonical form)"
    from oracle import level0
    key = (name, value, diag_mode, tuple(origin))
    if key not in _oracle:
        A = field(name)[0]
        O = level0.march3d(A, value, diag_mode=diag_mode, origin=origin)
        ko = level0.edge_keys_from_pairs(O["pairs"], A.shape)
        _oracle[key] = (O, ko, level0.canonical_level0(ko, O["xyz"], O["tris"]))
    return _oracle[key]


def assert_mesh_is_oracle(ctx, counts, name, value, diag_mode, origin):
    "the comparison of tests/test_gpu_level0.py::check_against_oracle: counts, every edge id, every triangle key triple, coordinates"
    from oracle import level0
    O, ko, co = oracle_mesh(name, value, diag_mode, origin)
    xyz, keys, tris = ctx.download_level0(counts)
    keys = keys.astype(np.int64)
    ch = level0.canonical_level0(keys, xyz, tris.astype(np.int64))
    assert counts["n_vertices"] == len(ko) and counts["n_triangles"] == len(O["tris"])
    assert counts["n_border_voxels"] == O["nborder_mixed"]
    assert len(np.unique(keys)) == len(keys)
    assert np.array_equal(co[0], ch[0])
    err = np.abs(ch[1].astype(np.float64) - co[1])
    assert np.all(err <= REL_TOL * np.abs(co[1]) + ABS_FLOOR), err.max()
    assert np.array_equal(co[2], ch[2])


def modes():
    from contourist_amd import _ffi
    return [(_ffi.CX_DIAG_CPYTHON310, 1, (0, 0, 0)), (_ffi.CX_DIAG_CANONICAL, 0, (3, 5, 7)), (_ffi.CX_DIAG_CPYTHON310, 1, (-1, -2, -3))]


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_slim_records_mesh_is_the_oracles(name):
    """the default path (slim records) with ccap == n_cells exactly, both diagonal modes, a positive and a negative origin; one
    record short answers CX_ERR_CAPACITY, and the synchronous call then grows and gives the same mesh"""
    from contourist_amd import _ffi
    A, v = field(name)
    loose = _ffi.Context(0)
    try:
        loose.upload_grid(A)
        counts = loose.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        assert loose.level0_path() == 1
        assert_mesh_is_oracle(loose, counts, name, v, 1, (0, 0, 0))
    finally:
        loose.close()
    nc = counts["n_cells"]
    print(name, counts)
    if name == "tiny":
        assert 0 < nc < 64
    if name == "odd":
        assert nc > 64 and nc % 64 != 0
    exact = _ffi.Context(0)
    try:
        exact.reserve(nc, counts["n_vertices"], counts["n_triangles"])
        exact.upload_grid(A)
        for flags, diag_mode, origin in modes():
            exact.set_origin(*origin)
            c = exact.extract3d(v, flags)
            assert exact.level0_path() == 1
            assert c["n_cells"] == nc
            assert_mesh_is_oracle(exact, c, name, v, diag_mode, origin)
    finally:
        exact.close()
    short = _ffi.Context(0)
    try:
        short.reserve(nc - 1, counts["n_vertices"], counts["n_triangles"])
        short.upload_grid(A)
        short.extract3d_async(v, _ffi.CX_DIAG_CPYTHON310)
        with pytest.raises(_ffi.CxError) as e:
            short.counts()
        assert e.value.code == _ffi.CX_ERR_CAPACITY
        c = short.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        assert c == counts
        assert_mesh_is_oracle(short, c, name, v, 1, (0, 0, 0))
    finally:
        short.close()


# ---- full records on demand: the seeded selection after a default extraction ------------------------------------------------------
SEEDED = {"tiny": (1.3, 2.1), "odd": (0.1, -0.35), "noise": (0.0, 0.4)}
_kept = {}


def kept_by_oracle(name, value, picks):
    "end points on crossing edges of the oracle's mesh, and the edge-id triples of the triangles the restated search keeps"
    from oracle import seeds
    key = (name, value)
    if key not in _kept:
        A = field(name)[0]
        O, ko, _ = oracle_mesh(name, value, 1, (0, 0, 0))
        rng = np.random.RandomState(17)
        pick = rng.choice(len(ko), size=picks, replace=False)
        eps = [[tuple(int(x) for x in O["pairs"][p][:3]), tuple(int(x) for x in O["pairs"][p][3:])] for p in pick]
        want, _ = seeds.select(A, value, eps, ko, O["tris"])
        _kept[key] = (eps, _triples(ko, O["tris"][want]))
    return _kept[key]


def _triples(keys, tris):
    "triangles as rows of edge ids, each row sorted, rows sorted (as oracle.level0.canonical_level0): independent of the numbering"
    t = np.sort(np.asarray(keys, dtype=np.int64)[np.asarray(tris, dtype=np.int64).reshape(-1, 3)], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))] if len(t) else t


def extract_and_select(ctx, name, value, flags):
    eps, want = kept_by_oracle(name, value, 2)
    counts = ctx.extract3d(value, flags)
    got = ctx.select_seeded(eps)
    tk, _ = ctx.seeded_masks(counts)
    _, keys, tris = ctx.download_level0(counts)
    assert got["triangles_kept"] == len(want) == int(tk.sum())
    assert np.array_equal(_triples(keys, tris[tk]), want)
    return got


@pytest.mark.parametrize("name", sorted(SEEDED))
def test_full_records_on_demand(name):
    """extract, select, extract at another isovalue, select again: the selection walks 16-byte records, which the vertex stage
    rebuilds over the slim ones"""
    from contourist_amd import _ffi
    A = field(name)[0]
    fresh = {}
    for v in SEEDED[name]:      # what a fresh context answers
        c = _ffi.Context(0)
        try:
            c.upload_grid(A)
            fresh[v] = extract_and_select(c, name, v, _ffi.CX_DIAG_CPYTHON310)
        finally:
            c.close()
    ctx = _ffi.Context(0)
    try:
        ctx.upload_grid(A)
        for v in SEEDED[name] + SEEDED[name][:1]:
            assert extract_and_select(ctx, name, v, _ffi.CX_DIAG_CPYTHON310) == fresh[v]
            assert ctx.level0_path() == 1
        # the default and the generic path in turn on one context: slim records, full records from separate reservations, ...
        for n, v in enumerate(SEEDED[name] * 2):
            flags = _ffi.CX_DIAG_CPYTHON310 | (_ffi.CX_KERNEL_GENERIC if n % 2 else 0)
            assert extract_and_select(ctx, name, v, flags) == fresh[v]
            assert ctx.level0_path() == (0 if n % 2 else 1)
        for n, v in enumerate(SEEDED[name] * 2):
            flags = _ffi.CX_DIAG_CPYTHON310 | (0 if n % 2 else _ffi.CX_KERNEL_GENERIC)
            assert extract_and_select(ctx, name, v, flags) == fresh[v]
    finally:
        ctx.close()


# ---- one context through shapes with more and fewer chunks of totals, the levels call, the generic path, regrown capacities ---------
def _gentle(shape, f=1.0):
    i, j, k = _axes(shape)
    n0, n1, n2 = shape
    return (np.sin(f * 4.1 * i / n0 + 0.4) * np.cos(f * 3.3 * j / n1) + 0.8 * np.sin(f * 3.9 * k / n2 + 1.0)).astype(np.float32)


# A: 140 workgroups of the stream kernel = 560 streaming waves = 3 chunks of totals, 124 k vertices (inside the capacities a context
# reserves by itself for this shape); B: 320 = 1280 = 5 chunks, 207 k vertices; C: A's shape with 364 k vertices, more than the
# capacities any step before it has grown to
CHUNK_FIELDS = {"A": lambda: _gentle((40, 100, 300)), "B": lambda: _gentle((64, 160, 300)), "C": lambda: _gentle((40, 100, 300), 3.0)}
_chunk = {}
_expect = {}


def chunk_field(name):
    if name not in _chunk:
        _chunk[name] = CHUNK_FIELDS[name]()
    return _chunk[name]


def _steps():
    from contourist_amd import _ffi
    d = _ffi.CX_DIAG_CPYTHON310
    a = ("x", "A", 0.1, d)
    return [a, a, a, ("x", "B", 0.1, d), a, ("levels", "A", (0.1, -0.2), d), a, ("x", "A", 0.1, d | _ffi.CX_KERNEL_GENERIC), a,
            ("x", "C", 0.1, d), a]


def _canonical(ctx, counts):
    from oracle import level0
    xyz, keys, tris = ctx.download_level0(counts)
    return level0.canonical_level0(keys.astype(np.int64), xyz, tris.astype(np.int64))


def expected(step):
    "what a fresh context answers to one step"
    from contourist_amd import _ffi
    if step not in _expect:
        ctx = _ffi.Context(0)
        try:
            ctx.upload_grid(chunk_field(step[1]))
            if step[0] == "levels":
                _expect[step] = ctx.extract3d_levels(step[2], step[3])
            else:
                c = ctx.extract3d(step[2], step[3])
                _expect[step] = (c, _canonical(ctx, c))
        finally:
            ctx.close()
    return _expect[step]


def enqueue(ctx, step):
    ctx.upload_grid(chunk_field(step[1]))
    if step[0] == "x":
        ctx.extract3d_async(step[2], step[3])


def finish(ctx, step):
    "-> True when the first attempt overflowed the capacities and the synchronous call grew them and ran again"
    from contourist_amd import _ffi
    if step[0] == "levels":
        assert ctx.extract3d_levels(step[2], step[3]) == expected(step)
        return False
    grew = False
    try:
        c = ctx.counts()
    except _ffi.CxError as e:
        assert e.code == _ffi.CX_ERR_CAPACITY
        c = ctx.extract3d(step[2], step[3])
        grew = True
    want_counts, want_mesh = expected(step)
    assert c == want_counts, (step, c, want_counts)
    got = _canonical(ctx, c)
    assert np.array_equal(got[0], want_mesh[0]) and np.array_equal(got[2], want_mesh[2]) and np.array_equal(got[1], want_mesh[1])
    return grew


def test_chunk_totals_one_context():
    "the same shape again and again, a larger one, the levels call, the generic path and a regrown extraction in between"
    from contourist_amd import _ffi
    ctx = _ffi.Context(0)
    try:
        grown = []
        for step in _steps():
            enqueue(ctx, step)
            grown.append(finish(ctx, step))
        # B and C overflow what the steps before them had reserved; nothing else does (totals left over from an earlier
        # extraction would show as counts beyond the capacities)
        assert grown == [False, False, False, True, False, False, False, False, False, True, False]
    finally:
        ctx.close()


def test_chunk_totals_two_contexts_two_streams():
    "two contexts, each on its own stream, taking the steps in turn with both extractions in flight"
    from contourist_amd import _ffi
    a, b = _ffi.Context(0), _ffi.Context(0)
    try:
        steps = _steps()
        for n, step in enumerate(steps):
            other = steps[(n + 3) % len(steps)]
            enqueue(a, step)
            enqueue(b, other)
            finish(a, step)
            finish(b, other)
    finally:
        a.close()
        b.close()


# ---- kernel times -----------------------------------------------------------------------------------------------------------------
def test_timing_events_made_at_enable():
    from contourist_amd import _ffi
    A = _smooth((64, 64, 64), 12)
    small = _smooth((16, 16, 16), 13)
    ctx = _ffi.Context(0)
    try:
        ctx.upload_grid(A)
        ctx.extract3d(0.1, 1)                      # buffers sized, kernels loaded
        ctx.extract3d(0.1, 1)
        t = ctx.timing_read()
        assert t["n"] == 0 and t["total_ms"] == 0.0          # timing off: nothing recorded
        N = 5
        for rep in range(2):                                  # enable, read, enable again
            ctx.timing_enable(True)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(N):
                ctx.extract3d(0.1, 1)
            wall_ms = (time.perf_counter() - t0) * 1e3
            t = ctx.timing_read()
            print("timing", rep, t, "wall ms", wall_ms)
            assert t["n"] == N
            four = [t["stream_ms"], t["scan_ms"], t["cells_ms"], t["emit_ms"]]
            assert all(math.isfinite(x) and x > 0.0 for x in four), four
            assert sum(four) <= wall_ms
            assert t["classify_ms"] == pytest.approx(sum(four[:3]), rel=1e-5) and t["total_ms"] == pytest.approx(sum(four), rel=1e-5)
            assert ctx.timing_read()["n"] == 0               # read and gone
            ctx.timing_enable(False)
            ctx.extract3d(0.1, 1)
            assert ctx.timing_read()["n"] == 0
        # the generic path: classify and triangle stage, nothing for the scan
        ctx.timing_enable(True)
        for _ in range(N):
            ctx.extract3d(0.1, 1 | _ffi.CX_KERNEL_GENERIC)
        t = ctx.timing_read()
        assert t["n"] == N and t["stream_ms"] > 0.0 and t["emit_ms"] > 0.0 and math.isfinite(t["total_ms"])
        # more extractions than the pool holds: the ones beyond it run untimed
        ctx.upload_grid(small)
        ctx.extract3d(0.1, 1)
        ctx.timing_enable(True)
        for _ in range(300):
            ctx.extract3d_async(0.1, 1)
        c = ctx.counts()
        t = ctx.timing_read()
        assert t["n"] == 256 and math.isfinite(t["total_ms"]) and t["total_ms"] > 0.0
        assert c == ctx.extract3d(0.1, 1)
        ctx.timing_enable(False)
    finally:
        ctx.close()
