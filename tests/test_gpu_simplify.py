"""Simplification of the Level-1 mesh by vertex clustering on the device (cx_simplify.hip) against tests/simplify_ref.py, the numpy
and Python-int restatement of the header's section "simplification", run on the mesh downloaded BEFORE the call (points, triangles
in device order, vertex labels, normals).  The orientation step only reverses whole components: rows are compared after undoing the
reversal the components' `flipped` reports.

Noise field of the clean case: synthetic.smooth_noise_host((96, 96, 96), seed 7, 6), the generator's rough setting the components
tests use.  The share of triangles whose cross product the reference's np.allclose area rule sits on the edge of is computed on the
host in float64 with the operands of the cross product swapped (cross(A-C, B-C) against -cross(B-C, A-C): the oracle against
itself); the test prints it and asserts that it is 0.0 for this seed (the issue's cap is 1e-3), so no triangle is excluded from the
comparison: triangle set and points are compared exactly."""
import json

import numpy as np
import pytest

import simplify_ref as R

pytestmark = pytest.mark.gpu

CELLS = [1.5, 2.0, 4.0, (2.0, 3.0, 5.0)]


def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def _ball(shape, c, r):
    I, J, K = _grid(shape)
    return np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - r


def _field(name):
    if name == "sphere":
        return _ball((48, 48, 48), (23.3, 22.6, 24.2), 15.4).astype(np.float32), 0.0
    if name == "two_blobs":
        return np.minimum(_ball((48, 40, 40), (13.2, 19.4, 20.1), 9.3), _ball((48, 40, 40), (34.3, 20.6, 18.9), 7.1)).astype(np.float32), 0.0
    if name == "noise":
        from contourist_amd import synthetic
        return synthetic.smooth_noise_host((96, 96, 96), 7, 6).astype(np.float32), 0.8
    if name == "two_blobs_u8":
        A, _v = _field("two_blobs")
        return np.clip(np.round(128.0 + 8.0 * A.astype(np.float64)), 0, 255).astype(np.uint8), 128.5
    raise KeyError(name)


def _context(A, value):
    from contourist_amd import _ffi
    ctx = _ffi.Context()
    ctx.upload_grid_native(A)
    counts = ctx.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    assert counts["n_vertices"] > 0
    return ctx, ctx.postprocess3d()


def _source(ctx, post, normals):
    pts, tris = ctx.download_level1(post)
    tl, vl = ctx.level1_component_labels()
    N = ctx.level1_normals(post) if normals else None
    return pts, tris, vl, N


def _after(ctx, out, n_old):
    p2, t2 = ctx.download_level1(out)
    table = ctx.level1_components()
    tl2, vl2 = ctx.level1_component_labels()
    return dict(points=p2, triangles=t2, rows=R.unflip(t2, tl2, table["flipped"]), keys=ctx.download_level1_keys(out),
                map=ctx.level1_simplify_map(n_old), table=table, tl=tl2, vl=vl2)


def _check_exact(ctx, post, corner, cell, by_component, normals=False, what=""):
    "CX_SIMPLIFY_NO_CLEAN against the restatement: everything bit for bit / row for row"
    from contourist_amd import _ffi
    pts, tris, vl, N = _source(ctx, post, normals)
    ref = R.simplify(pts, tris, corner, cell, by_component, normals=N, vlab=vl)
    flags = _ffi.CX_SIMPLIFY_NO_CLEAN | (0 if by_component else _ffi.CX_SIMPLIFY_ACROSS_COMPONENTS) | (_ffi.CX_SIMPLIFY_NORMALS if normals else 0)
    out = ctx.level1_simplify(cell, flags)
    G = _after(ctx, out, len(pts))
    assert out["q"] == ref["q"] and out["n_clusters"] == ref["n_clusters"] and out["n_distinct"] == ref["n_distinct"], (what, out, ref["n_clusters"], ref["n_distinct"])
    assert out["clamped"] == ref["clamped"] == 0
    assert out["n_vertices"] == len(ref["points"]) and out["n_triangles"] == len(ref["triangles"]) <= out["n_distinct"], what
    assert out["n_components"] == len(G["table"])
    assert G["points"].tobytes() == ref["points"].tobytes(), what
    assert np.array_equal(G["rows"], ref["triangles"]), what
    assert np.array_equal(G["map"], ref["map"]) and np.array_equal(G["keys"], ref["keys"]), what
    return out, ref, G


# ---- 1. exact parity without clean -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "two_blobs", "noise", "two_blobs_u8"])
def test_exact_parity_without_clean(name):
    A, value = _field(name)
    corner = tuple(n - 1 for n in A.shape)
    ctx, post = _context(A, value)
    try:
        for cell in CELLS:
            for by_component in (True, False):
                post = ctx.postprocess3d()
                out, ref, G = _check_exact(ctx, post, corner, cell, by_component, what="%s cell %s by_component %s" % (name, cell, by_component))
                print(name, cell, by_component, "->", out["n_vertices"], "vertices", out["n_triangles"], "triangles of", post["n_triangles"])
    finally:
        ctx.close()


def _slab_maker():
    from contourist_amd import tetrahedral
    A, value = _field("two_blobs")
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    m.MAX_SAMPLES_PER_EXTRACTION = 40 * 40 * 12
    assert m._in_slabs()
    return m, A


def test_exact_parity_on_a_slab_marched_volume():
    "a cx_postprocess3d_mesh source: keys are vertex indices, normals are not available"
    from contourist_amd import _ffi
    m, A = _slab_maker()
    corner = tuple(n - 1 for n in A.shape)
    for cell in CELLS:
        for by_component in (True, False):
            m._post = None
            ctx = m._ensure_post(True)
            assert m._slab_counts["n_slabs"] >= 2
            _check_exact(ctx, m._post, corner, cell, by_component, what="slabs cell %s" % (cell,))
    # CX_SIMPLIFY_NORMALS on such a source: UNSUPPORTED, the mesh untouched
    m._post = None
    ctx = m._ensure_post(True)
    before = [a.tobytes() for a in ctx.download_level1(m._post)]
    with pytest.raises(NotImplementedError):
        ctx.level1_simplify(2.0, _ffi.CX_SIMPLIFY_NORMALS)
    assert [a.tobytes() for a in ctx.download_level1(m._post)] == before
    assert m.simplify(cell=2.0)["n_triangles"] > 0                      # normals="auto" leaves them out here
    with pytest.raises(NotImplementedError):
        m.vertex_normals()


# ---- 2. with clean -----------------------------------------------------------------------------------------------------------
def _edge_share(P, T):
    "share of triangles the np.allclose area rule decides differently with the operands of the cross product swapped"
    A, B, C = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    d1 = np.all(np.abs(np.cross(A - C, B - C)) <= 1e-8, axis=1)
    d2 = np.all(np.abs(np.cross(B - C, A - C)) <= 1e-8, axis=1)
    return float(np.count_nonzero(d1 != d2)) / max(1, len(T))


@pytest.mark.parametrize("name", ["sphere", "two_blobs", "noise"])
def test_with_clean_against_the_oracle(name):
    from oracle import postpass
    A, value = _field(name)
    corner = tuple(n - 1 for n in A.shape)
    ctx, post = _context(A, value)
    try:
        for cell in ([2.0, (2.0, 3.0, 5.0)] if name == "noise" else CELLS):
            post = ctx.postprocess3d()
            pts, tris, vl, _n = _source(ctx, post, False)
            ref = R.simplify(pts, tris, corner, cell, True, vlab=vl)
            out = ctx.level1_simplify(cell, 0)
            G = _after(ctx, out, len(pts))
            old = ref["raw_old"]
            share = _edge_share(ref["raw_points"], ref["raw_triangles"])
            print(name, cell, "share of triangles on the edge of the area rule:", share)
            assert share == 0.0      # (for the named seed no triangle sits on the edge of the rule: nothing is excluded below)
            x2, t2 = postpass.clean(ref["raw_points"], ref["raw_triangles"], np.stack([old, old, old], axis=1))
            want = set(map(tuple, np.asarray(t2).tolist()))
            got = set(map(tuple, G["rows"].tolist()))
            assert G["points"].tobytes() == np.asarray(x2).tobytes() and got == want, (name, cell, len(got ^ want))
            assert out["n_clusters"] == ref["n_clusters"] and out["n_distinct"] == ref["n_distinct"]
            assert out["n_triangles"] <= out["n_distinct"]
    finally:
        ctx.close()


# ---- 3. carried normals ------------------------------------------------------------------------------------------------------
def test_carried_normals():
    A, value = _field("sphere")
    corner = tuple(n - 1 for n in A.shape)
    c0, r0 = np.array((23.3, 22.6, 24.2)), 15.4
    ctx, post = _context(A, value)
    worst = 0.0
    try:
        for cell in CELLS:
            post = ctx.postprocess3d()
            src_table = ctx.level1_components()
            assert len(src_table) == 1
            out, ref, G = _check_exact(ctx, post, corner, cell, True, normals=True, what="normals cell %s" % (cell,))
            N = ctx.level1_normals(out)
            err = float(np.abs(N - ref["normals"]).max())
            worst = max(worst, err)
            assert err <= 1e-12
            delta = (0.5, 1.25, 2.0)
            Nd = ctx.level1_normals(out, delta)
            assert np.abs(Nd - R.scaled_normals(N, delta)).max() <= 1e-12
            # derived: the members of a cluster lie within one cell diagonal d of each other on the sphere, so their radial directions,
            # the direction of their mean and the normalised sum of their normals lie in a cone whose opening is the angle the chord
            # d subtends at radius r0, 2 asin(d / 2 r0) (d / r0 to second order; the interpolation's error is far below either)
            diag = float(np.linalg.norm(np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,))))
            radial = G["points"] - c0
            radial /= np.linalg.norm(radial, axis=1)[:, None]
            # the field grows outward, so the gradient is radial; the source's normals are s * g / |g| with s = -1 where the orientation
            # step reversed the source's (only) component, and the carried normals keep that sign
            sign = -1.0 if int(src_table["flipped"][0]) else 1.0
            ang = np.arccos(np.clip(np.sum(sign * N * radial, axis=1), -1.0, 1.0))
            bound = 2.0 * np.arcsin(diag / (2.0 * r0))
            print("cell", cell, "largest angle to the radial direction", float(ang.max()), "bound", bound, "margin", bound - float(ang.max()))
            assert float(ang.max()) <= bound
            # a second simplification carries the carried normals on
            src = ctx.level1_normals(out)
            pts, tris = ctx.download_level1(out)
            tl, vl = ctx.level1_component_labels()
            ref2 = R.simplify(pts, tris, corner, 6.0, True, normals=src, vlab=vl)
            from contourist_amd import _ffi
            out2 = ctx.level1_simplify(6.0, _ffi.CX_SIMPLIFY_NO_CLEAN | _ffi.CX_SIMPLIFY_NORMALS)
            assert ctx.download_level1(out2)[0].tobytes() == ref2["points"].tobytes()
            assert np.abs(ctx.level1_normals(out2) - ref2["normals"]).max() <= 1e-12
        print("carried normals: worst difference to the restatement", worst)
        # without the flag the normals calls answer UNSUPPORTED afterwards
        post = ctx.postprocess3d()
        out = ctx.level1_simplify(2.0, 0)
        with pytest.raises(NotImplementedError):
            ctx.level1_normals(out)
    finally:
        ctx.close()


# ---- 4. readers --------------------------------------------------------------------------------------------------------------
def test_readers(tmp_path):
    torch = pytest.importorskip("torch")
    from contourist_amd import tetrahedral, mesh_io
    A, value = _field("two_blobs")
    S = tetrahedral.TriangulatedIsosurfaces([0.5, 1.0, -2.0], None, [0.5, 1.0, 2.0], A, value, [])
    S.search_for_endpoints()
    full = S.get_points_and_triangles()
    counts = S.simplify(cell=2.0)
    assert set(counts) == {"n_vertices", "n_triangles", "n_components", "n_clusters", "cell", "clamped"} and counts["cell"] == (2.0, 2.0, 2.0)
    assert 0 < counts["n_triangles"] < len(full[1]) and counts["n_components"] == 2
    maker = S.contour_maker
    ctx = maker.context()
    pg, td = ctx.download_level1(maker._post)
    world = S.grid.from_grid_coordinates(pg)
    P, T = S.get_points_and_triangles()
    assert len(P) == counts["n_vertices"] and len(T) == counts["n_triangles"]
    assert np.array_equal(P, world) and np.array_equal(T, np.array(sorted(map(tuple, td.tolist())), dtype=np.int32))
    Pd, Td = S.get_points_and_triangles(device=True)
    assert np.array_equal(Pd.cpu().numpy(), world) and np.array_equal(Td.cpu().numpy(), td)
    N = S.vertex_normals()
    assert N.shape == (len(P), 3) and np.abs(np.linalg.norm(N, axis=1) - 1.0).max() < 1e-12
    m = S.simplify_map()
    assert len(m) == len(full[0]) and m.max() == len(P) - 1 and np.array_equal(S.simplify_map(device=True).cpu().numpy(), m)
    for fmt, nrm in (("ply", None), ("ply_normals", N)):
        dev, host = str(tmp_path / (fmt + "_d.ply")), str(tmp_path / (fmt + "_h.ply"))
        S.write_mesh(dev, fmt)
        mesh_io.write_ply(host, world, td, normals=nrm)
        assert open(dev, "rb").read() == open(host, "rb").read(), fmt
    for fmt, nrm in (("gltf", None), ("gltf_normals", N)):
        dev, host = str(tmp_path / (fmt + "_d.gltf")), str(tmp_path / (fmt + "_h.gltf"))
        S.write_mesh(dev, fmt)
        mesh_io.write_gltf_bin(host, world, td, normals=nrm)
        assert open(dev[:-5] + ".bin", "rb").read() == open(host[:-5] + ".bin", "rb").read(), fmt
        a, b = json.load(open(dev)), json.load(open(host))
        assert a["accessors"] == b["accessors"] and a["bufferViews"] == b["bufferViews"], fmt
    with pytest.raises(NotImplementedError):
        S.vertex_values(A)
    # components() after the simplification against a host union-find
    table = S.components()
    tl, vl = ctx.level1_component_labels()
    rtl, rvl = R.vertex_labels(td, len(pg))
    assert np.array_equal(tl, rtl) and np.array_equal(vl, rvl) and np.array_equal(np.bincount(rtl), table["triangles"])
    # keep_components after simplify: mesh and carried normals follow
    big = int(np.argmax(table["triangles"]))
    kept = S.keep_components(largest=1)
    assert kept["n_triangles"] == int(table["triangles"][big]) and kept["n_components"] == 1
    P1, T1 = S.get_points_and_triangles()
    sel = rvl == big
    assert np.array_equal(P1, world[sel]) and np.array_equal(S.vertex_normals(), N[sel])
    # simplify after keep_components
    S2 = tetrahedral.TriangulatedIsosurfaces([0.5, 1.0, -2.0], None, [0.5, 1.0, 2.0], A, value, [])
    S2.search_for_endpoints()
    S2.keep_components(largest=1)
    m2 = S2.contour_maker
    pts, tris = m2.context().download_level1(m2._post)
    c2 = S2.simplify(cell=2.0, clean=False)
    ref = R.simplify(pts, tris, tuple(n - 1 for n in A.shape), 2.0)
    assert c2["n_components"] == 1 and m2.context().download_level1(m2._post)[0].tobytes() == ref["points"].tobytes()


# ---- 5. target_triangles -----------------------------------------------------------------------------------------------------
def test_target_triangles():
    from contourist_amd import tetrahedral, _ffi
    A, value = _field("sphere")
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    full = m.get_points_and_triangles()
    ctx = m.context()
    before = [a.tobytes() for a in ctx.download_level1(m._post)]
    dry = ctx.level1_simplify(3.0, _ffi.CX_SIMPLIFY_COUNT_ONLY)
    assert dry["n_vertices"] == 0 and dry["n_triangles"] == 0 and dry["n_clusters"] > 0 and dry["n_distinct"] > 0
    assert [a.tobytes() for a in ctx.download_level1(m._post)] == before            # a dry run leaves the download unchanged
    n = len(full[1]) // 6
    counts = m.simplify(target_triangles=n)
    assert 0 < counts["n_triangles"] <= n
    search = m._simplify_search
    assert 2 <= len(search) <= 16 and search[0][0] == float(max(m.corner))
    chosen = counts["cell"][0]
    ok = [c for c, got in search if got <= n]
    assert chosen == min(ok)
    smaller = [(c, got) for c, got in search if c < chosen]
    assert smaller and max(smaller)[1] > n                                            # the next smaller cell of the bisection exceeds n
    assert chosen - max(smaller)[0] < 1.0 / 16.0 or len(search) == 16
    print("target", n, "-> cell", chosen, counts["n_triangles"], "triangles after", len(search), "dry runs")
    # a dry run leaves the map of the last simplification alone as well
    map_before = m.simplify_map()
    ctx.level1_simplify(3.0, _ffi.CX_SIMPLIFY_COUNT_ONLY)
    assert np.array_equal(m.simplify_map(), map_before) and map_before.max() == counts["n_vertices"] - 1
    m2 = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    m2.get_points_and_triangles()
    with pytest.raises(_ffi.CxError) as e0:                                           # no simplification yet: the library's answer
        m2.simplify_map()
    assert e0.value.code == _ffi.CX_ERR_STATE
    # the largest cell (max corner) holds this whole sphere: it reaches 0 triangles, so only a target below that is out of reach
    with pytest.raises(ValueError) as e:
        m2.simplify(target_triangles=-1)
    assert "still leaves 0 triangles" in str(e.value)
    assert len(m2.get_points_and_triangles()[1]) == len(full[1])                      # (the failed call ran dry runs only)
    assert m2.simplify(target_triangles=1)["n_triangles"] <= 1
    # a ball about the far corner of the array, cut open by three faces: the vertices ON those faces (coordinate == corner) lie in the
    # next cell of the largest lattice, so the largest cell still leaves triangles; one fewer than it reaches is out of reach
    B = _ball((48, 48, 48), (47.0, 47.0, 47.0), 20.3).astype(np.float32)
    m3 = tetrahedral.GridContour3d((47, 47, 47), B, 0.0)
    m3.get_points_and_triangles()
    reached = m3.context().level1_simplify(47.0, _ffi.CX_SIMPLIFY_COUNT_ONLY)["n_distinct"]
    print("corner ball: the largest cell reaches", reached, "triangles")
    with pytest.raises(ValueError) as e:
        m3.simplify(target_triangles=reached - 1)
    assert "still leaves %d triangles" % reached in str(e.value)
    assert m3.simplify(target_triangles=reached)["n_triangles"] <= reached
    with pytest.raises(ValueError):
        m2.simplify()
    with pytest.raises(ValueError):
        m2.simplify(cell=2.0, target_triangles=100)


# ---- 6. routes and state -----------------------------------------------------------------------------------------------------
def test_routes_and_state():
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, synthetic, tetrahedral
    A, value = _field("two_blobs")
    corner = tuple(n - 1 for n in A.shape)
    fresh = _ffi.Context()
    fresh.upload_grid_native(A)
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    with pytest.raises(_ffi.CxError) as e:
        fresh.level1_simplify(2.0)
    assert e.value.code == _ffi.CX_ERR_INVALID
    fresh.set_reference_corner(corner)
    fresh.shard_begin(0, A.shape[0] - 1)
    fresh.shard_finish([], [])
    with pytest.raises(NotImplementedError):
        fresh.level1_simplify(2.0)
    fresh.set_reference_corner((0, 0, 0))
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    post = fresh.postprocess3d()
    before = [a.tobytes() for a in fresh.download_level1(post)]
    with pytest.raises(_ffi.CxError) as e:                                            # too many cells: INVALID, the mesh untouched
        fresh.level1_simplify(1e-4)
    assert e.value.code == _ffi.CX_ERR_INVALID and "smallest admissible cell" in str(e.value)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_ffi.CxError) as e:
            fresh.level1_simplify(bad)
        assert e.value.code == _ffi.CX_ERR_INVALID
    assert [a.tobytes() for a in fresh.download_level1(post)] == before
    with pytest.raises(_ffi.CxError) as e:
        fresh.level1_simplify_map(post["n_vertices"])
    assert e.value.code == _ffi.CX_ERR_STATE
    # all in one cell: no triangle survives
    out = fresh.level1_simplify(1000.0)
    assert out["n_triangles"] == 0 and out["n_vertices"] == 0 and out["n_clusters"] == 2 and out["n_distinct"] == 0
    assert np.all(fresh.level1_simplify_map(post["n_vertices"]) == -1) and len(fresh.level1_components()) == 0
    # an empty mesh in gives an empty mesh out
    out = fresh.level1_simplify(2.0)
    assert (out["n_vertices"], out["n_triangles"], out["n_clusters"], out["n_distinct"]) == (0, 0, 0, 0)
    # a new post-pass restores the full mesh and its normals
    post = fresh.postprocess3d()
    N0 = fresh.level1_normals(post)
    fresh.level1_simplify(3.0)
    post2 = fresh.postprocess3d()
    assert [a.tobytes() for a in fresh.download_level1(post2)] == before and fresh.level1_normals(post2).tobytes() == N0.tobytes()
    # a 4-D pass on the same context takes the memory of the orientation tables
    B = synthetic.moving_blobs_torch((20, 20, 20, 12), 3, torch.device("cuda", 0))
    fresh.adopt_device_grid4d(B.data_ptr(), tuple(B.shape), keepalive=B)
    fresh.extract4d(0.5)
    fresh.postprocess4d()
    with pytest.raises(_ffi.CxError) as e3:
        fresh.level1_simplify(2.0)
    assert e3.value.code == _ffi.CX_ERR_STATE and "orientation tables" in str(e3.value)
    fresh.close()
    # the Python layer: vertex_values() raises after simplify, a new march restores everything
    m = tetrahedral.GridContour3d(corner, A, value)
    full = m.get_points_and_triangles()
    m.simplify(cell=3.0)
    with pytest.raises(NotImplementedError):
        m.vertex_values(A)
    assert len(m.get_points_and_triangles()[1]) < len(full[1])
    m.march(force=True)
    again = m.get_points_and_triangles()
    assert np.array_equal(again[0], full[0]) and np.array_equal(again[1], full[1])
    assert np.array_equal(m.vertex_values(A).shape, (len(full[0]),)) and m.vertex_normals().shape == full[0].shape


def test_levels():
    "LevelResult.simplify / simplify_map / mesh / vertex_normals on the levels of MultiLevelIsosurfaces"
    from contourist_amd import tetrahedral, _ffi
    A, _v = _field("two_blobs")
    corner = tuple(n - 1 for n in A.shape)
    mins, delta = np.array([0.5, 1.0, -2.0]), np.array([0.5, 1.0, 2.0])
    M = tetrahedral.MultiLevelIsosurfaces(mins, None, delta, A, [-1.0, 0.5])
    seen = 0
    for lv in M.levels():
        ctx = lv._ctx()
        with pytest.raises(_ffi.CxError) as e:
            lv.simplify_map()
        assert e.value.code == _ffi.CX_ERR_STATE
        pts, tris = ctx.download_level1(lv._post)
        tl, vl = ctx.level1_component_labels()
        N = ctx.level1_normals(lv._post)
        ref = R.simplify(pts, tris, corner, (2.0, 3.0, 5.0), True, normals=N, vlab=vl)
        counts = lv.simplify(cell=(2.0, 3.0, 5.0), clean=False)
        assert set(counts) == set(_ffi.SIMPLIFY_KEYS) and counts["n_clusters"] == ref["n_clusters"] and counts["n_triangles"] == len(ref["triangles"])
        P, T = lv.mesh()
        assert np.array_equal(P, ref["points"] * delta + mins) and len(T) == len(ref["triangles"])
        assert np.array_equal(lv.simplify_map(), ref["map"])
        assert np.abs(lv.vertex_normals() - R.scaled_normals(ref["normals"], delta)).max() <= 1e-12
        assert len(lv.components()) == counts["n_components"]
        with pytest.raises(NotImplementedError):
            lv.vertex_values(A)
        seen += 1
    assert seen == 2


# ---- 7. reproducibility ------------------------------------------------------------------------------------------------------
def test_bit_identical():
    from contourist_amd import _ffi
    A, value = _field("noise")
    blobs = []
    for k in range(2):
        ctx, post = _context(A, value)
        for again in range(2):
            post = ctx.postprocess3d()
            n_old = post["n_vertices"]
            out = ctx.level1_simplify((2.0, 3.0, 5.0), _ffi.CX_SIMPLIFY_NORMALS)
            p, t = ctx.download_level1(out)
            blobs.append((p.tobytes(), t.tobytes(), ctx.download_level1_keys(out).tobytes(), ctx.level1_simplify_map(n_old).tobytes(),
                          ctx.level1_normals(out).tobytes(), ctx.level1_components().tobytes(), json.dumps(out, sort_keys=True)))
        ctx.close()
    assert all(b == blobs[0] for b in blobs[1:])


# ---- 8. full size ------------------------------------------------------------------------------------------------------------
def test_bench_field_at_full_size():
    """the 512^3 bench field, cell 4, with normals: cluster and distinct-triangle counts against the restatement's clustering stage
    (vectorised numpy), positions on a 1/64 sample of the clusters with Python integers.  (That a second call allocates nothing is checked at small
    size, tests/test_gpu_buffers.py.)"""
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, synthetic
    dev = torch.device("cuda", 0)
    A = synthetic.smooth_noise_torch((512,) * 3, 1235, 1400, dev)
    ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
        ctx.extract3d(0.0, 1)
        post = ctx.postprocess3d(0)
        corner = (511, 511, 511)
        pts, tris = ctx.download_level1(post)
        tl, vl = ctx.level1_component_labels()
        out = ctx.level1_simplify(4.0, _ffi.CX_SIMPLIFY_NORMALS | _ffi.CX_SIMPLIFY_NO_CLEAN)     # (no clean: every position is a cluster's own mean)
        cid, first, _k = R.clusters(pts, vl, corner, 4.0)
        M, ok = R.remap_triangles(tris, cid)
        assert out["n_clusters"] == len(first) and out["n_distinct"] == int(ok.sum()) and out["clamped"] == 0
        assert out["n_triangles"] <= out["n_distinct"]
        p2, t2 = ctx.download_level1(out)
        m = ctx.level1_simplify_map(len(pts))
        keys = ctx.download_level1_keys(out).astype(np.int64)
        assert len(p2) == out["n_vertices"] and len(t2) == out["n_triangles"] and t2.min() >= 0 and t2.max() < len(p2)
        assert m.max() == len(p2) - 1 and m.min() >= -1
        live = m >= 0
        assert np.all(np.abs(pts[live] - p2[m[live]]) <= 4.0)                          # every old vertex within the cell of its new one
        assert np.array_equal(np.floor(pts[live] / 4.0), np.floor(pts[keys[m[live]]] / 4.0))
        N = ctx.level1_normals(out)
        assert N.shape == p2.shape and np.abs(np.linalg.norm(N, axis=1) - 1.0).max() < 1e-9
        # positions of every 64th surviving vertex: the exact mean of its members
        sample = np.arange(0, len(p2), 64)
        cl = cid[keys[sample]]
        want, _c = R.exact_means(pts, cid, len(first), corner, R.q_of(corner), only=[int(c) for c in cl])
        size_ref = np.bincount(cid[cid >= 0], minlength=len(first))[cl]
        size_gpu = np.bincount(m[live], minlength=len(p2))[sample]
        same = size_ref == size_gpu
        assert same.all() and p2[sample].tobytes() == want[cl].tobytes()
        print("512^3 cell 4:", post["n_triangles"], "->", out["n_triangles"], "triangles,", out["n_clusters"], "clusters,", out["n_vertices"], "vertices,",
              out["n_components"], "components; sample", len(sample), "positions exact")
    finally:
        ctx.close()
        del A
        torch.cuda.empty_cache()
