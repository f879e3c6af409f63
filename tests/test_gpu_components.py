"""Components of the Level-1 mesh on the device (cx_comp.hip): labels, per-component measures and filtering against a float64
numpy / scipy restatement of the definitions in include/contourist_hip.h ("components") on the downloaded mesh.

Oracle: components = connected components of the graph "triangles that share an undirected edge"; ids by smallest triangle index
in device order; terms by the header's formulas in float64; sums with math.fsum.  It equals the orientation step's components
where no edge is used by more than two triangles, which is asserted on every test mesh (a property of the input).  In the coarse
weld regime, where the weld pinches sheets together, the rule of the device is: every pair of triangles that share an edge is
linked whatever the edge's multiplicity (cxp_k_edges_link*: an edge with three or more triangles links all of them and carries no
relative winding), so the components are still those of the shared-edge graph; it is stated here, not tested against scipy.

Bound of the sums (assertion 2 of the issue): |gpu - fsum| <= n_c * 2^-(q+1) + 16 * 2^-53 * sum_i P_i, q as returned by the
library (every term is rounded once to a multiple of 2^-q or finer and the integers are added exactly), P_i the sum of the
absolute values of the products that make up triangle i's term.  Worst observed fraction of the bound: printed by every case."""
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


# ---- fields -----------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def _ball(shape, c, r):
    I, J, K = _grid(shape)
    return np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - r


def _fields(name):
    "-> (fp32 or uint8 samples, isovalue)"
    if name == "sphere":            # (a) one sphere, 64^3
        return _ball((64, 64, 64), (31.3, 30.6, 32.2), 20.4).astype(np.float32), 0.0
    if name == "two_spheres":       # (b) two disjoint spheres of different radius
        return np.minimum(_ball((64, 48, 48), (17.2, 23.4, 24.1), 12.3), _ball((64, 48, 48), (46.3, 24.6, 22.9), 9.1)).astype(np.float32), 0.0
    if name == "nested":            # (c) nested shells: f < 0 between the two radii
        r = _ball((41, 41, 41), (20.0, 20.0, 20.0), 0.0)
        return (-(r - 6.3) * (r - 12.6)).astype(np.float32), 0.0
    if name == "cut":               # (d) a sphere the array's rim cuts open
        return _ball((48, 48, 48), (3.3, 22.6, 25.2), 14.4).astype(np.float32), 0.0
    if name == "touching":          # (e) two octahedra that meet in ONE lattice point, where f == value exactly: the crossings of
        r = 5                       # the edges into that point coincide there and are welded into one vertex of both components
        shape = (4 * r + 9, 2 * r + 9, 2 * r + 9)           # (checked with oracle/level0.py + oracle/postpass.py: 2 components)
        I, J, K = _grid(shape)
        c = r + 4
        return np.minimum(abs(I - c) + abs(J - c) + abs(K - c), abs(I - c - 2 * r) + abs(J - c) + abs(K - c)).astype(np.float32) - np.float32(r), 0.0
    if name == "noise":             # (f) smooth noise, 96^3: hundreds of components, one dominant.  At 96^3 the weld buckets are 1/105 of a
        # voxel and a crossing close to a lattice point is welded to its neighbours there, which pinches sheets together (edges with
        # three triangles).  Samples that are INTEGERS within 20 of a half-integer isovalue keep every crossing at least
        # 0.5 / 40 = 1/80 of an edge away from both ends: no two crossings share a bucket, nothing is welded, and the condition on the
        # input holds (checked with oracle/level0.py + oracle/postpass.py: 242 components, the largest 1.10 M of 1.23 M triangles)
        from contourist_amd import synthetic
        N = synthetic.smooth_noise_host((96, 96, 96), 7, 6).astype(np.float64)
        return np.clip(np.round((N - 0.8) * 6.0), -20, 20).astype(np.float32), 0.5
    if name == "two_spheres_u8":    # (i) uint8 samples of (b)
        A, _v = _fields("two_spheres")
        return np.clip(np.round(128.0 + 8.0 * A.astype(np.float64)), 0, 255).astype(np.uint8), 128.5
    raise KeyError(name)



# ---- oracle -----------------------------------------------------------------------------------------------------------------
def _edge_table(tris, nv):
    "per triangle corner k the key of the undirected edge (v[k], v[k+1]); (keys (T,3), multiplicity of every key (T,3))"
    T = np.asarray(tris, dtype=np.int64)
    a, b = T, np.roll(T, -1, axis=1)
    keys = np.minimum(a, b) * nv + np.maximum(a, b)
    u, inv, cnt = np.unique(keys.ravel(), return_inverse=True, return_counts=True)
    return keys, cnt[inv].reshape(keys.shape)


def _components_of(tris, nv):
    "labels (T,) of the shared-edge graph, ids in ascending order of the smallest triangle index"
    T = np.asarray(tris, dtype=np.int64)
    nt = len(T)
    keys, _mult = _edge_table(T, nv)
    k = keys.ravel()
    t = np.repeat(np.arange(nt), 3)
    order = np.argsort(k, kind="stable")
    k, t = k[order], t[order]
    same = k[1:] == k[:-1]
    a, b = t[:-1][same], t[1:][same]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        _n, lab = connected_components(coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(nt, nt)), directed=False)
    except ImportError:           # a small union-find: minimum label over the edges, then pointer jumping, until nothing moves
        lab = np.arange(nt)
        while True:
            m = np.minimum(lab[a], lab[b])
            new = lab.copy()
            np.minimum.at(new, a, m)
            np.minimum.at(new, b, m)
            while True:
                jump = new[new]
                if np.array_equal(jump, new):
                    break
                new = jump
            if np.array_equal(new, lab):
                break
            lab = new
    first = np.full(int(lab.max()) + 1 if nt else 0, nt, dtype=np.int64)
    np.minimum.at(first, lab, np.arange(nt))
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[lab].astype(np.int32), np.sort(first)


def _oracle(pts, tris, corner, mins=None, delta=None):
    "dict of per-component arrays by the header's formulas, float64, sums with math.fsum; P_* the sums of the terms' |products|"
    P = np.asarray(pts, dtype=np.float64)
    T = np.asarray(tris, dtype=np.int64)
    nv, nt = len(P), len(T)
    keys, mult = _edge_table(T, nv)
    assert nt == 0 or mult.max() <= 2, "condition on the input: an edge of this mesh is used by more than two triangles"
    tl, first = _components_of(T, nv)
    nc = len(first)
    vl = np.full(nv, np.iinfo(np.int32).max, dtype=np.int32)
    for k in range(3):
        np.minimum.at(vl, T[:, k], tl)
    vl[vl == np.iinfo(np.int32).max] = -1
    d = np.ones(3) if delta is None else np.asarray(delta, dtype=np.float64)
    m = np.zeros(3) if mins is None else np.asarray(mins, dtype=np.float64)
    W = P * d + m if (mins is not None or delta is not None) else P
    o = (np.asarray(corner, dtype=np.float64) / 2.0) * d + m
    p0, p1, p2 = W[T[:, 0]], W[T[:, 1]], W[T[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    area = np.linalg.norm(np.cross(e1, e2), axis=1) / 2.0
    P_area = np.abs(e1).sum(axis=1) * np.abs(e2).sum(axis=1)
    a, b, c = p0 - o, p1 - o, p2 - o
    prods = [a[:, 0] * b[:, 1] * c[:, 2], a[:, 0] * b[:, 2] * c[:, 1], a[:, 1] * b[:, 2] * c[:, 0], a[:, 1] * b[:, 0] * c[:, 2],
             a[:, 2] * b[:, 0] * c[:, 1], a[:, 2] * b[:, 1] * c[:, 0]]
    vol = (prods[0] - prods[1] + prods[2] - prods[3] + prods[4] - prods[5]) / 6.0
    P_vol = sum(np.abs(x) for x in prods) / 6.0
    cen = (a + b + c) / 3.0                       # triangle centroids about o
    mom = area[:, None] * cen
    P_mom = P_area[:, None] * (np.abs(a) + np.abs(b) + np.abs(c)) / 3.0
    order = np.argsort(tl, kind="stable")
    bounds = np.searchsorted(tl[order], np.arange(nc + 1))
    R = dict(nc=nc, tl=tl, vl=vl, first=first, origin=o, W=W, triangles=np.bincount(tl, minlength=nc), vertices=np.bincount(vl[vl >= 0], minlength=nc),
             area=np.zeros(nc), volume=np.zeros(nc), moment=np.zeros((nc, 3)), P_area=np.zeros(nc), P_vol=np.zeros(nc), P_mom=np.zeros((nc, 3)),
             lo=np.zeros((nc, 3)), hi=np.zeros((nc, 3)), closed=np.zeros(nc, dtype=np.int32))
    for cidx in range(nc):
        rows = order[bounds[cidx]:bounds[cidx + 1]]
        R["area"][cidx] = math.fsum(area[rows]); R["volume"][cidx] = math.fsum(vol[rows])
        R["P_area"][cidx] = math.fsum(P_area[rows]); R["P_vol"][cidx] = math.fsum(P_vol[rows])
        for k in range(3):
            R["moment"][cidx, k] = math.fsum(mom[rows, k]); R["P_mom"][cidx, k] = math.fsum(P_mom[rows, k])
        V = W[T[rows].ravel()]
        R["lo"][cidx], R["hi"][cidx] = V.min(axis=0), V.max(axis=0)
        # exact edge count within the component: closed = every edge of its triangles is used an even number of times by them
        _u, cnt = np.unique(keys[rows].ravel(), return_counts=True)
        R["closed"][cidx] = int(np.all(cnt % 2 == 0))
    R["volume_all"], R["P_vol_all"] = math.fsum(vol), math.fsum(P_vol)
    return R


def _check_table(table, origin, q, R, what):
    "assertions 1 and 2 of the issue for one table against one oracle; -> worst observed fraction of the bound of the sums"
    nc = R["nc"]
    assert len(table) == nc
    assert np.array_equal(table["triangles"], R["triangles"]) and np.array_equal(table["vertices"], R["vertices"])
    assert np.array_equal(table["first_triangle"], R["first"])
    assert np.array_equal(table["closed"], R["closed"])
    assert np.array_equal(origin, R["origin"])
    assert table["bbox_lo"].tobytes() == R["lo"].tobytes() and table["bbox_hi"].tobytes() == R["hi"].tobytes()       # bit for bit
    n = R["triangles"].astype(np.float64)
    grid = n * 2.0 ** -(q + 1)
    b_area, b_vol, b_mom = grid + 16 * EPS * R["P_area"], grid + 16 * EPS * R["P_vol"], grid[:, None] + 16 * EPS * R["P_mom"]
    e_area, e_vol = np.abs(table["area"] - R["area"]), np.abs(table["volume"] - R["volume"])
    worst = max(float((e_area / b_area).max()), float((e_vol / b_vol).max())) if nc else 0.0
    print(what, "components", nc, "q", q, "worst |area err| / bound", float((e_area / b_area).max()) if nc else 0.0,
          "worst |volume err| / bound", float((e_vol / b_vol).max()) if nc else 0.0)
    assert np.all(e_area <= b_area) and np.all(e_vol <= b_vol)
    # the sum over the components against the whole mesh's volume, to the same bound
    total = math.fsum(table["volume"])
    assert abs(total - R["volume_all"]) <= n.sum() * 2.0 ** -(q + 1) + 16 * EPS * R["P_vol_all"]
    # centroid = o + M / A with the moments M about o summed like the other two: the quotient's error is at most
    # (b_mom + |M / A| * b_area) / A, doubled for the division and the addition of o and with their own roundings on top
    pos = R["area"] > 0
    cref = R["origin"] + R["moment"][pos] / R["area"][pos, None]
    rel = np.abs(R["moment"][pos] / R["area"][pos, None])
    b_cen = 2.0 * (b_mom[pos] + rel * b_area[pos, None]) / R["area"][pos, None] + 4 * EPS * (np.abs(R["origin"]) + rel)
    e_cen = np.abs(table["centroid"][pos] - cref)
    print(what, "worst |centroid err| / bound", float((e_cen / b_cen).max()) if pos.any() else 0.0)
    assert np.all(e_cen <= b_cen)
    assert np.all(table["centroid"][~pos] == 0.0)
    return worst


def _context(A, value):
    from contourist_amd import _ffi
    ctx = _ffi.Context()
    ctx.upload_grid_native(A)
    counts = ctx.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    assert counts["n_vertices"] > 0
    post = ctx.postprocess3d()
    return ctx, post


def _check_context(ctx, post, corner, what, mins=None, delta=None):
    "labels and table of a context's Level-1 mesh against the oracle on its download; -> (table, oracle, pts, tris)"
    pts, tris = ctx.download_level1(post)
    R = _oracle(pts, tris, corner, mins, delta)
    assert R["nc"] == post["n_components"]
    tl, vl = ctx.level1_component_labels()
    assert tl.dtype == np.int32 and vl.dtype == np.int32
    assert np.array_equal(tl, R["tl"]) and np.array_equal(vl, R["vl"])
    table, origin, q = ctx.level1_components(mins, delta, info=True)
    _check_table(table, origin, q, R, what)
    return table, R, pts, tris


# ---- 1 - 3: labels, counts, box, sums, physics -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "two_spheres", "nested", "cut", "touching", "noise", "two_spheres_u8"])
def test_components_against_the_oracle(name):
    A, value = _fields(name)
    corner = tuple(n - 1 for n in A.shape)
    ctx, post = _context(A, value)
    try:
        table, R, pts, tris = _check_context(ctx, post, corner, name)
        nc = len(table)
        if name == "sphere":
            assert nc == 1 and table["closed"][0] == 1 and table["volume"][0] > 0
            print("sphere: volume / (4/3 pi r^3)", table["volume"][0] / (4.0 / 3.0 * np.pi * 20.4 ** 3), "area / (4 pi r^2)", table["area"][0] / (4 * np.pi * 20.4 ** 2))
        if name in ("two_spheres", "two_spheres_u8"):
            assert nc == 2 and np.all(table["closed"] == 1) and np.all(table["volume"] > 0)
            assert table["triangles"][0] != table["triangles"][1]
        if name == "nested":
            assert nc == 2 and np.all(table["closed"] == 1)
            assert np.array_equal(np.sign(table["volume"]), np.sign(R["volume"])) and np.all(R["volume"] != 0)
        if name == "cut":
            assert nc == 1 and table["closed"][0] == 0
        if name == "touching":
            assert nc == 2 and np.all(table["closed"] == 1)
            both = np.zeros((len(pts), 2), dtype=bool)
            for k in range(3):
                both[tris[:, k], R["tl"]] = True
            assert int(both.all(axis=1).sum()) == 1                  # one vertex belongs to triangles of both components
            assert table["vertices"].sum() == len(pts)               # ... and is counted once, for the smaller id
        if name == "noise":
            assert nc >= 100 and table["triangles"].max() > 0.5 * len(tris)
        # flipped: the sign the normals take (tests/test_gpu_normals.py: s = -1 for the vertices of a reversed component)
        if A.dtype == np.float32 and name != "touching":       # (touching: f == value at lattice points, zero gradients there)
            from test_gpu_normals import _check_level1
            _N, s, _ = _check_level1(ctx, post, A.astype(np.float64), value)
            used = (R["vl"] >= 0) & (np.abs(_N).sum(axis=1) > 0)       # (a zero gradient has no sign)
            assert np.array_equal(s[used] < 0, table["flipped"][R["vl"][used]] == 1)
        # world coordinates: anisotropic spacing (g) on the two spheres, a shifted origin on the others
        mins, delta = ((-3.0, 0.25, 7.5), (0.5, 1.0, 2.0)) if name == "two_spheres" else ((1.5, -2.0, 0.125), (0.25, 0.25, 0.25))
        wtable, _R, _p, _t = _check_context(ctx, post, corner, name + " (world)", mins, delta)
        assert np.array_equal(wtable["triangles"], table["triangles"]) and np.array_equal(wtable["closed"], table["closed"])
        scale = float(np.prod(delta))
        assert np.allclose(wtable["volume"], table["volume"] * scale, rtol=1e-9, atol=1e-9 * scale)
    finally:
        ctx.close()


# ---- (h) routes without edge ids: refined points, a volume marched in slabs --------------------------------------------------
def test_refined_points_and_slabs():
    from contourist_amd import tetrahedral
    # field (a) as a callable: the sphere of radius 20.4 about (31.3, 30.6, 32.2) on the 64^3 lattice, crossing points refined on the host
    S = tetrahedral.TriangulatedIsosurfaces([0.0] * 3, [62.0] * 3, [1.0] * 3,
                                            lambda x, y, z: np.sqrt((x - 31.3) ** 2 + (y - 30.6) ** 2 + (z - 32.2) ** 2) - 20.4, 0.0, [], linear_interpolate=False)
    S.search_for_endpoints()
    maker = S.contour_maker
    table = S.components()
    ctx = maker.context()
    pts, tris = ctx.download_level1(maker._post)
    corner = [int(c) for c in maker.corner] if maker.voxel_range is None else [int(h) - int(l) for l, h in zip(*maker.voxel_range)]
    R = _oracle(pts, tris, corner, S.grid.mins, S.grid.delta)
    wt, origin, q = ctx.level1_components(S.grid.mins, S.grid.delta, info=True)
    assert wt.tobytes() == table.tobytes()
    _check_table(table, origin, q, R, "refined")
    assert len(table) == 1 and table["closed"][0] == 1 and table["volume"][0] > 0
    exact = 4.0 / 3.0 * np.pi * 20.4 ** 3
    print("refined sphere: volume / exact", table["volume"][0] / exact)
    assert abs(table["volume"][0] / exact - 1.0) < 0.01
    # slabs: the limit lowered as tests/test_gpu_fullsize.py does
    A, value = _fields("two_spheres")
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    m.MAX_SAMPLES_PER_EXTRACTION = 48 * 48 * 16
    assert m._in_slabs()
    table = m.components()
    assert m._slab_counts["n_slabs"] >= 2
    ctx = m.context()
    _check_context(ctx, m._post, tuple(n - 1 for n in A.shape), "slabs")
    assert len(table) == 2 and np.all(table["closed"] == 1) and np.all(table["volume"] > 0)
    # host labels follow the sorted rows of get_points_and_triangles
    p, t = m.get_points_and_triangles()
    tl, vl = m.component_labels()
    Rh = _oracle(p, t, tuple(n - 1 for n in A.shape))
    # (ids are defined by the device order; as sets of triangles the components are the same)
    assert len(np.unique(np.stack([tl, Rh["tl"]], axis=1), axis=0)) == 2
    assert np.array_equal(np.bincount(tl), table["triangles"])


# ---- 4. reproducibility ------------------------------------------------------------------------------------------------------
def test_tables_are_bit_identical():
    A, value = _fields("noise")
    blobs = []
    for _ in range(2):
        ctx, post = _context(A, value)
        try:
            t1 = ctx.level1_components()
            ctx.level1_components((0.0, 1.0, 2.0), (0.5, 0.5, 0.5))          # another mapping in between: the cache is rebuilt
            t2 = ctx.level1_components()
            assert t1.tobytes() == t2.tobytes()
            blobs.append(t1.tobytes() + ctx.level1_component_labels()[0].tobytes())
        finally:
            ctx.close()
    assert blobs[0] == blobs[1]


# ---- 5. keep_components ------------------------------------------------------------------------------------------------------
def _host_filter(pts, keys, tris, tl, keep):
    kt = keep[tl]
    T = tris[kt]
    used = np.zeros(len(pts), dtype=bool)
    used[T.ravel()] = True
    new = np.cumsum(used) - 1
    return pts[used], keys[used], new[T].astype(np.int32), used


@pytest.mark.parametrize("name,selector", [("noise", dict(largest=1)), ("two_spheres", dict(mask=[False, True])), ("noise", dict(min_triangles=40, closed=True))])
def test_keep_components(name, selector, tmp_path):
    from contourist_amd import tetrahedral, mesh_io, surface_geometry
    A, value = _fields(name)
    corner = tuple(n - 1 for n in A.shape)
    ref = tetrahedral.GridContour3d(corner, A, value)             # an untouched second object
    rctx = ref._ensure_post()
    pts0, tris0 = rctx.download_level1(ref._post)
    keys0 = rctx.download_level1_keys(ref._post)
    table0 = ref.components()
    tl0, _vl0 = rctx.level1_component_labels()
    normals0 = ref.vertex_normals()
    keep = surface_geometry.select_components(table0, **selector)
    assert keep.any() and not keep.all()
    P, K, T, used = _host_filter(pts0, keys0, tris0, tl0, keep)

    m = tetrahedral.GridContour3d(corner, A, value)
    ones = m.keep_components(mask=np.ones(len(table0), dtype=bool))            # all ones: nothing changes, bit for bit
    ctx = m.context()
    assert ones == dict(n_vertices=len(pts0), n_triangles=len(tris0), n_components=len(table0))
    p1, t1 = ctx.download_level1(m._post)
    assert p1.tobytes() == pts0.tobytes() and t1.tobytes() == tris0.tobytes() and ctx.download_level1_keys(m._post).tobytes() == keys0.tobytes()
    assert m.components().tobytes() == table0.tobytes()
    counts = m.keep_components(**selector)
    assert counts == dict(n_vertices=len(P), n_triangles=len(T), n_components=int(keep.sum()))
    p2, t2 = ctx.download_level1(m._post)
    assert p2.tobytes() == P.tobytes() and ctx.download_level1_keys(m._post).tobytes() == K.tobytes()          # vertex order preserved
    assert np.array_equal(surface_geometry.sort_rows(t2), surface_geometry.sort_rows(T)) and np.array_equal(t2, T)
    # the kept records, bitwise; only first_triangle follows the new numbering.  (The sign of a normal is read from the FILTERED tables: a
    # vertex that two components with different flips share takes the flip of a kept one.  No mesh here has such a vertex.)
    table2 = m.components()
    want = table0[keep].copy()
    want["first_triangle"] = (np.cumsum(keep[tl0]) - 1)[table0["first_triangle"][keep]]
    assert table2.tobytes() == want.tobytes()
    tl2, vl2 = ctx.level1_component_labels()
    assert np.array_equal(tl2, (np.cumsum(keep) - 1)[tl0[keep[tl0]]])
    _check_context(ctx, m._post, corner, name + " (filtered)")
    # every reader serves the filtered mesh
    gp, gt = m.get_points_and_triangles()
    assert np.array_equal(gp, P) and np.array_equal(gt, surface_geometry.sort_rows(T))
    assert m.vertex_normals().tobytes() == normals0[used].tobytes()
    B = np.arange(A.size, dtype=np.float32).reshape(A.shape)
    assert m.vertex_values(B).tobytes() == ref.vertex_values(B)[used].tobytes()
    for fmt in ("ply", "ply_normals"):
        path = str(tmp_path / ("kept_" + fmt + ".ply"))
        info = m.write_mesh(path, fmt, (1.0, 2.0, 3.0), (0.5, 0.25, 2.0))
        got = mesh_io.read_ply(path)
        assert info["n_vertices"] == len(P) and info["n_triangles"] == len(T)
        assert np.array_equal(got[0], P * np.array([0.5, 0.25, 2.0]) + np.array([1.0, 2.0, 3.0])) and np.array_equal(got[1], T)
    for fmt in ("gltf_bin", "gltf_bin_normals"):
        path = str(tmp_path / ("kept_" + fmt + ".bin"))
        info = m.write_mesh(path, fmt)
        blob = open(path, "rb").read()
        assert info["n_vertices"] == len(P) and len(blob) == len(P) * (24 if fmt.endswith("normals") else 12) + len(T) * 12
        assert np.array_equal(np.frombuffer(blob[:len(P) * 12], dtype="<f4").reshape(-1, 3), P.astype(np.float32))
        assert np.array_equal(np.frombuffer(blob[-len(T) * 12:], dtype="<u4").reshape(-1, 3), T.astype(np.uint32))
    # a second keep on the result, then nothing at all
    if counts["n_components"] > 1:
        again = m.keep_components(largest=1)
        assert again["n_components"] == 1 and again["n_triangles"] == int(table2["triangles"].max())
        _check_context(ctx, m._post, corner, name + " (filtered twice)")
    none = m.keep_components(mask=np.zeros(m._post["n_components"], dtype=bool))
    assert (none["n_vertices"], none["n_triangles"], none["n_components"]) == (0, 0, 0)
    gp, gt = m.get_points_and_triangles()
    assert len(gp) == 0 and len(gt) == 0 and len(m.components()) == 0
    assert m.vertex_normals().shape == (0, 3)
    # the other object was not touched
    assert ref.components().tobytes() == table0.tobytes()


def test_python_api_world_and_levels(tmp_path):
    torch = pytest.importorskip("torch")
    from contourist_amd import tetrahedral
    A, value = _fields("two_spheres")
    mins, delta = (-3.0, 0.25, 7.5), (0.5, 1.0, 2.0)
    S = tetrahedral.TriangulatedIsosurfaces(mins, None, delta, A, value, [])
    S.search_for_endpoints()
    table, tl, vl = S.components(device=True)
    maker = S.contour_maker
    ctx = maker.context()
    pts, tris = ctx.download_level1(maker._post)
    R = _oracle(pts, tris, tuple(n - 1 for n in A.shape), mins, delta)
    wt, origin, q = ctx.level1_components(mins, delta, info=True)
    assert wt.tobytes() == table.tobytes()
    _check_table(table, origin, q, R, "world")
    assert tl.is_cuda and tl.dtype == torch.int32 and np.array_equal(tl.cpu().numpy(), R["tl"]) and np.array_equal(vl.cpu().numpy(), R["vl"])
    dp, dt = S.get_points_and_triangles(device=True)
    assert len(dt) == len(tl) and len(dp) == len(vl)
    htl, hvl = S.component_labels()
    wp, wtris = S.get_points_and_triangles()
    assert len(htl) == len(wtris) and np.array_equal(np.bincount(htl), table["triangles"]) and np.array_equal(hvl, R["vl"])
    small = int(np.argmin(table["area"]))
    counts = S.keep_components(min_area=float(table["area"].max()))           # world units: only the larger sphere passes
    assert counts["n_components"] == 1 and counts["n_triangles"] == int(table["triangles"][1 - small])
    assert len(S.get_points_and_triangles()[1]) == counts["n_triangles"]
    from contourist_amd import mesh_io
    gpath = str(tmp_path / "kept.gltf")
    mesh_io.write_gltf_device(S, gpath, normals=True)          # the Delta3DContour "gltf_normals" route serves the filtered mesh
    kp, kt = S.contour_maker.context().download_level1(S.contour_maker._post)
    blob = open(str(tmp_path / "kept.bin"), "rb").read()
    assert len(blob) == len(kp) * 24 + len(kt) * 12 and len(kt) == counts["n_triangles"]
    assert np.array_equal(np.frombuffer(blob[-len(kt) * 12:], dtype="<u4").reshape(-1, 3), kt.astype(np.uint32))
    after = S.components()
    for field in ("triangles", "vertices", "area", "volume", "centroid", "bbox_lo", "bbox_hi", "flipped", "closed"):
        assert after[field].tobytes() == table[[1 - small]][field].tobytes(), field
    # the levels of MultiLevelIsosurfaces
    M = tetrahedral.MultiLevelIsosurfaces(mins, None, delta, A, [-1.5, 0.0])
    seen = 0
    for level in M.levels():
        v, points, triangles = level
        t = level.components()
        assert len(t) == 2 and int(t["triangles"].sum()) == len(triangles) and np.all(t["closed"] == 1) and np.all(t["volume"] > 0)
        ltl, lvl = level.component_labels()
        assert np.array_equal(np.bincount(ltl), t["triangles"]) and len(lvl) == len(points)
        kept = level.keep_components(largest=1)
        fp, ft = level.mesh()
        assert kept["n_components"] == 1 and len(ft) == int(t["triangles"].max()) == kept["n_triangles"] and len(fp) == kept["n_vertices"]
        assert level.vertex_normals().shape == (len(fp), 3)
        seen += 1
    assert seen == 2


# ---- 6. routes ---------------------------------------------------------------------------------------------------------------
def test_routes():
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, synthetic
    A, value = _fields("two_spheres")
    fresh = _ffi.Context()
    fresh.upload_grid_native(A)
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    with pytest.raises(_ffi.CxError) as e:                                  # before any post-pass: what the normals raise
        fresh.level1_components()
    assert e.value.code == _ffi.CX_ERR_INVALID
    with pytest.raises(_ffi.CxError) as e2:
        fresh.level1_normals(dict(n_vertices=0))
    assert e2.value.code == _ffi.CX_ERR_INVALID
    # the sharded post-pass
    fresh.set_reference_corner(tuple(n - 1 for n in A.shape))
    fresh.shard_begin(0, A.shape[0] - 1)
    fresh.shard_finish([], [])
    for call in (fresh.level1_components, fresh.level1_component_labels, lambda: fresh.level1_keep_components([True, True])):
        with pytest.raises(NotImplementedError):
            call()
    # a 4-D pass on the same context takes the memory of the orientation tables
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    post = fresh.postprocess3d()
    assert len(fresh.level1_components()) == 2 == post["n_components"]
    B = synthetic.moving_blobs_torch((20, 20, 20, 12), 3, torch.device("cuda", 0))
    fresh.adopt_device_grid4d(B.data_ptr(), tuple(B.shape), keepalive=B)
    fresh.extract4d(0.5)
    fresh.postprocess4d()
    with pytest.raises(_ffi.CxError) as e3:
        fresh.level1_components()
    assert e3.value.code == _ffi.CX_ERR_STATE and "orientation tables" in str(e3.value)
    fresh.close()


# ---- 7. full size ------------------------------------------------------------------------------------------------------------
def test_bench_field_at_full_size():
    """the 512^3 bench field: nc == out_counts[4], the triangles and vertices of the components add up, and the largest
    component's counts against a union-find on the downloaded triangles"""
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, synthetic
    dev = torch.device("cuda", 0)
    A = synthetic.smooth_noise_torch((512,) * 3, 1235, 1400, dev)
    ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.adopt_device_grid(A.data_ptr(), tuple(A.shape), keepalive=A)
        ctx.extract3d(0.0, 1)
        post = ctx.postprocess3d(0)
        table, origin, q = ctx.level1_components(info=True)
        tl, vl = ctx.level1_component_labels()
        nv, nt = post["n_vertices"], post["n_triangles"]
        assert len(table) == post["n_components"]
        assert int(table["triangles"].sum()) == nt and int(table["vertices"].sum()) + int((vl < 0).sum()) == nv
        assert np.array_equal(np.bincount(tl, minlength=len(table)), table["triangles"])
        _pts, tris = ctx.download_level1(post)
        lab, first = _components_of(tris, nv)
        del _pts
        big = int(np.argmax(table["triangles"]))
        assert len(first) == len(table) and np.array_equal(first, table["first_triangle"])
        assert int(np.bincount(lab)[big]) == int(table["triangles"][big])
        vmin = np.full(nv, np.iinfo(np.int32).max, dtype=np.int32)
        for k in range(3):
            np.minimum.at(vmin, tris[:, k], lab)
        assert int((vmin == big).sum()) == int(table["vertices"][big])
        print("512^3: components", len(table), "largest", int(table["triangles"][big]), "of", nt, "triangles, q", q,
              "area", float(table["area"][big]), "volume", float(table["volume"][big]), "closed", int(table["closed"][big]))
        kept = ctx.level1_keep_components(np.arange(len(table)) == big)
        assert kept == dict(n_vertices=int(table["vertices"][big]), n_triangles=int(table["triangles"][big]), n_components=1)
        t2 = ctx.level1_components()
        want = table[[big]].copy()
        want["first_triangle"] = 0 if big == 0 else int((lab[:int(table["first_triangle"][big])] == big).sum())
        assert t2.tobytes() == want.tobytes()
    finally:
        ctx.close()
        del A
        torch.cuda.empty_cache()
