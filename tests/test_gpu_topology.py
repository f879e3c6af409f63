"""Topology of the Level-1 mesh on the device (cx_topo.hip): the table, the loop table and the loop-vertex array against
tests/topology_ref.py run on the downloaded mesh and the downloaded device-order labels.  Everything is an integer: every comparison
is for equality."""
import numpy as np
import pytest

import topology_meshes as meshes
import topology_ref
from test_gpu_components import _ball, _context, _fields, _grid

pytestmark = pytest.mark.gpu


def _torus(shape, c, R, r):
    I, J, K = _grid(shape)
    return (np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2) - R) ** 2 + (K - c[2]) ** 2 - r * r


def _field(name):
    "-> (samples, isovalue)"
    if name == "sphere32":
        return _ball((32, 32, 32), (15.3, 14.6, 16.2), 10.4).astype(np.float32), 0.0
    if name == "torus":
        return _torus((40, 40, 20), (19.4, 19.7, 9.6), 11.3, 4.6).astype(np.float32), 0.0     # (at (19.3, 19.6, 9.7) the weld pinches it)
    if name == "tube":              # a cylinder along axis 0 that leaves the array through both end faces
        I, J, K = _grid((24, 24, 24))
        return (np.sqrt((J - 11.3) ** 2 + (K - 12.4) ** 2) - 6.4).astype(np.float32), 0.0
    if name == "sheet":             # a tilted plane: one long boundary loop around it
        I, J, K = _grid((64, 64, 8))
        return (0.31 * I + 0.17 * J + K - 4.3).astype(np.float32), 0.0
    if name in ("octahedron", "octahedron_small"):      # radius 1.5: exactly one wave of 64 triangles; radius 1.0: a partial wave
        I, J, K = _grid((8, 8, 8))
        return (abs(I - 3.3) + abs(J - 3.6) + abs(K - 4.2) - (1.5 if name == "octahedron" else 1.0)).astype(np.float32), 0.0
    if name == "sphere_and_torus":
        A = _torus((40, 40, 44), (19.3, 19.6, 9.7), 11.3, 4.6)
        return np.minimum(A, _ball((40, 40, 44), (19.3, 19.6, 31.2), 8.4)).astype(np.float32), 0.0
    if name == "cut_and_whole":
        return np.minimum(_ball((48, 48, 48), (3.3, 22.6, 25.2), 14.4), _ball((48, 48, 48), (33.1, 24.4, 23.7), 9.3)).astype(np.float32), 0.0
    return _fields(name)


def _check(ctx, post, what):
    "the device's three arrays against the reference on the downloaded mesh -> (table, loops, vertices, components table)"
    _pts, tris = ctx.download_level1(post)
    tl, _vl = ctx.level1_component_labels()
    want = topology_ref.topology(tris, tl)
    table = ctx.level1_topology()
    loops, verts = ctx.level1_boundary_loops()
    print(what, "nt", len(tris), "components", len(table), "loops", len(loops), "boundary edges", len(verts),
          "euler", table["euler"][:4].tolist(), "genus", table["genus"][:4].tolist(), "b", table["boundary_loops"][:4].tolist())
    assert table.dtype == topology_ref.TOPOLOGY_DTYPE and loops.dtype == topology_ref.LOOP_DTYPE and verts.dtype == np.int32
    assert len(table) == len(want[0]) == post["n_components"]
    for name in table.dtype.names:
        assert np.array_equal(table[name], want[0][name]), name
    assert table.tobytes() == want[0].tobytes()
    assert loops.tobytes() == want[1].tobytes()
    assert np.array_equal(verts, want[2])
    assert int(table["triangles"].sum()) == len(tris) and int(table["boundary_edges"].sum()) == len(verts)
    # the relation to the existing record
    comp = ctx.level1_components()
    whole = (table["boundary_edges"] == 0) & (table["nonmanifold_edges"] == 0)
    cut = (table["boundary_edges"] > 0) & (table["nonmanifold_edges"] == 0)
    assert np.all(comp["closed"][whole] == 1) and np.all(comp["closed"][cut] == 0)
    assert np.array_equal(comp["triangles"], table["triangles"])
    return table, loops, verts, comp


@pytest.mark.parametrize("name", ["sphere32", "torus", "cut", "tube", "sheet", "touching", "nested", "two_spheres_u8", "noise", "octahedron", "octahedron_small"])
def test_marched_meshes_against_the_reference(name):
    A, value = _field(name)
    ctx, post = _context(A, value)
    try:
        table, loops, verts, comp = _check(ctx, post, name)
        nv, nt = post["n_vertices"], post["n_triangles"]
        if name == "sphere32":
            assert len(table) == 1 and (table["euler"][0], table["genus"][0], table["boundary_loops"][0]) == (2, 0, 0)
        if name == "torus":
            assert len(table) == 1 and table["genus"][0] == 1 and table["euler"][0] == 0
        if name == "cut":
            assert len(table) == 1 and (table["boundary_loops"][0], table["euler"][0]) == (1, 1) and loops["simple"].tolist() == [1]
        if name == "tube":
            assert len(table) == 1 and (table["boundary_loops"][0], table["euler"][0], table["genus"][0]) == (2, 0, 0)
        if name == "sheet":
            assert len(loops) == 1 and loops["simple"][0] == 1 and loops["count"][0] > 128 and table["euler"][0] == 1      # (172 edges: 344 darts, two workgroups)
        if name == "touching":
            assert table["euler"].tolist() == [2, 2] and int(table["vertices"].sum()) == nv + 1
            assert int(comp["vertices"].sum()) == nv
        if name in ("nested", "two_spheres_u8"):
            assert table["euler"].tolist() == [2, 2] and table["genus"].tolist() == [0, 0] and len(loops) == 0
        if name == "noise":
            assert len(table) == 242
        if name == "octahedron":
            assert nt <= 64 and table["euler"].tolist() == [2]
        if name == "octahedron_small":
            assert nt < 64 and table["euler"].tolist() == [2]
    finally:
        ctx.close()


def test_empty_mesh():
    from contourist_amd import _ffi
    A, _value = _field("sphere32")
    ctx = _ffi.Context()
    try:
        ctx.upload_grid_native(A)
        counts = ctx.extract3d(1.0e9, _ffi.CX_DIAG_CPYTHON310)               # above every sample
        assert counts["n_vertices"] == 0
        ctx.postprocess3d()
        table = ctx.level1_topology()
        loops, verts = ctx.level1_boundary_loops()
        assert len(table) == 0 and len(loops) == 0 and len(verts) == 0
        assert table.dtype == _ffi.TOPOLOGY_DTYPE and loops.dtype == _ffi.LOOP_DTYPE
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["book", "moebius", "pinched_wheel"])
def test_hand_made_meshes(name):
    "the only cases that reach nonmanifold_edges > 0 and nonsimple_loops > 0 for certain"
    from contourist_amd import _ffi
    P, T = getattr(meshes, name)()
    ctx = _ffi.Context()
    try:
        post = ctx.postprocess3d_mesh(P, T, (16, 16, 16), flags=1 | 4)        # no clean | arbitrary windings
        assert post["n_triangles"] == len(T) and post["n_vertices"] == len(P)
        table, loops, verts, _comp = _check(ctx, post, name)
        assert len(table) == 1
        if name == "book":
            assert (table["nonmanifold_edges"][0], table["genus"][0], table["nonsimple_loops"][0]) == (1, -1, 1)
        if name == "moebius":
            assert (table["euler"][0], table["boundary_loops"][0], table["genus"][0]) == (0, 1, -1) and loops["simple"].tolist() == [1]
        if name == "pinched_wheel":
            assert (table["vertices"][0], table["edges"][0], table["triangles"][0], table["euler"][0]) == (13, 30, 16, -1)
            assert sorted(loops["simple"].tolist()) == [0, 1] and table["nonsimple_loops"][0] == 1
    finally:
        ctx.close()


def test_repeatable_and_cached():
    blobs = []
    A, value = _field("cut_and_whole")
    for _ in range(2):
        ctx, post = _context(A, value)
        try:
            first = ctx.level1_topology().tobytes() + b"".join(x.tobytes() for x in ctx.level1_boundary_loops())
            again = ctx.level1_topology().tobytes() + b"".join(x.tobytes() for x in ctx.level1_boundary_loops())
            assert first == again
            blobs.append(first)
        finally:
            ctx.close()
    assert blobs[0] == blobs[1] and len(blobs[0]) > 0


def test_after_keep_components():
    from contourist_amd import tetrahedral
    A, value = _field("noise")
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    before = m.topology()
    big = int(np.argmax(before["triangles"]))
    counts = m.keep_components(largest=1)
    assert counts["n_components"] == 1
    after = m.topology()
    assert after.tobytes() == before[[big]].tobytes()                      # the kept record, unchanged
    _check(m.context(), m._post, "noise (largest kept)")                   # the loops are renumbered: the reference on the new mesh


def test_after_simplify():
    from contourist_amd import tetrahedral
    A, value = _field("torus")
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    assert m.topology()["genus"].tolist() == [1]
    m.simplify(cell=3)
    table, _loops, _verts, _comp = _check(m.context(), m._post, "torus (cell 3)")
    print("simplified torus: genus", table["genus"].tolist(), "non-manifold edges", table["nonmanifold_edges"].tolist())


def test_python_api():
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, tetrahedral
    # genus=1 keeps the torus
    A, value = _field("sphere_and_torus")
    mins, delta = (-3.0, 0.25, 7.5), (0.5, 1.0, 2.0)
    S = tetrahedral.TriangulatedIsosurfaces(mins, None, delta, A, value, [])
    S.search_for_endpoints()
    table = S.topology()
    assert sorted(table["genus"].tolist()) == [0, 1] and table.dtype == _ffi.TOPOLOGY_DTYPE
    torus = int(np.argmax(table["genus"]))
    dev = S.topology(device=True)
    assert dev.is_cuda and dev.dtype == torch.int32 and dev.cpu().numpy().tobytes() == table.tobytes()
    counts = S.keep_components(genus=1)
    assert counts["n_components"] == 1 and counts["n_triangles"] == int(table["triangles"][torus])
    assert S.topology().tobytes() == table[[torus]].tobytes()
    # boundary_loops=0 keeps the whole sphere; the loops of the cut one as world points
    A, value = _field("cut_and_whole")
    S = tetrahedral.TriangulatedIsosurfaces(mins, None, delta, A, value, [])
    S.search_for_endpoints()
    table = S.topology()
    assert sorted(table["boundary_loops"].tolist()) == [0, 1]
    loops, verts, points = S.boundary_loops()
    P, _T = S.get_points_and_triangles()
    assert len(loops) == 1 and len(points) == 1 and points[0].shape == (int(loops["count"][0]), 3)
    assert np.array_equal(points[0], np.asarray(P)[verts[:int(loops["count"][0])]])
    dl, dv = S.boundary_loops(device=True)
    assert dl.is_cuda and dv.is_cuda and dl.cpu().numpy().tobytes() == loops.tobytes() and np.array_equal(dv.cpu().numpy(), verts)
    whole = int(np.argmin(table["boundary_loops"]))
    counts = S.keep_components(boundary_loops=0)
    assert counts["n_components"] == 1 and counts["n_triangles"] == int(table["triangles"][whole])
    assert len(S.boundary_loops()[0]) == 0
    # range selectors, nothing dropped
    assert S.keep_components(genus=(0, 5), boundary_loops=(0, 3))["n_components"] == 1
    # the levels of MultiLevelIsosurfaces
    A, _value = _field("cut_and_whole")
    M = tetrahedral.MultiLevelIsosurfaces(mins, None, delta, A, [-1.5, 0.0])
    seen = 0
    for level in M.levels():
        _v, points, triangles = level
        t = level.topology()
        ctx = level._ctx()
        tl, _vl = ctx.level1_component_labels()
        want = topology_ref.topology(ctx.download_level1(level._post)[1], tl)
        assert t.tobytes() == want[0].tobytes() and int(t["triangles"].sum()) == len(triangles)
        loops, verts, lp = level.boundary_loops()
        assert loops.tobytes() == want[1].tobytes() and np.array_equal(verts, want[2]) and len(lp) == len(loops) == 1
        seen += 1
    assert seen == 2


def test_routes_and_memory():
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, synthetic
    A, value = _fields("two_spheres")
    live0 = _ffi.device_bytes()[0]
    fresh = _ffi.Context()
    fresh.upload_grid_native(A)
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    for call in (fresh.level1_topology, fresh.level1_boundary_loops):
        with pytest.raises(_ffi.CxError) as e:                              # before any post-pass
            call()
        assert e.value.code == _ffi.CX_ERR_INVALID
    fresh.set_reference_corner(tuple(n - 1 for n in A.shape))               # the sharded post-pass
    fresh.shard_begin(0, A.shape[0] - 1)
    fresh.shard_finish([], [])
    for call in (fresh.level1_topology, fresh.level1_boundary_loops):
        with pytest.raises(NotImplementedError):
            call()
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    post = fresh.postprocess3d()
    before = _ffi.device_bytes(fresh.handle)[0]
    assert len(fresh.level1_topology()) == 2 == post["n_components"]
    assert _ffi.device_bytes(fresh.handle)[0] > before                      # the edge table is counted
    B = synthetic.moving_blobs_torch((20, 20, 20, 12), 3, torch.device("cuda", 0))      # a 4-D pass takes the orientation tables
    fresh.adopt_device_grid4d(B.data_ptr(), tuple(B.shape), keepalive=B)
    fresh.extract4d(0.5)
    fresh.postprocess4d()
    for call in (fresh.level1_topology, fresh.level1_boundary_loops):
        with pytest.raises(_ffi.CxError) as e3:
            call()
        assert e3.value.code == _ffi.CX_ERR_STATE
    fresh.close()
    assert _ffi.device_bytes()[0] == live0
