"""Vertex normals from the field's gradient and a second grid sampled at the vertices (cx_attr.hip), Level 0 and Level 1,
against float64 numpy restatements of the definition in include/contourist_hip.h ("vertex attributes")."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24


def _sines(shape=(40, 36, 44), seed=3):
    rng = np.random.default_rng(seed)
    g0, g1, g2 = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
    return (np.sin(3.1 * g0 + 0.4) * np.cos(2.7 * g1) + 0.8 * np.sin(3.9 * g2 + 1.0) + 0.05 * rng.standard_normal(shape)).astype(np.float32)


def _fields():
    "name -> (sample array in its own type, isovalue)"
    rng = np.random.default_rng(11)
    S = _sines()
    F = {
        "sines": (S, 0.1),
        "noise": (rng.standard_normal((28, 30, 32)).astype(np.float32), 0.1),
        "ragged": (_sines((9, 7, 3), seed=5), 0.1),                      # rows shorter than 4 samples: the generic classify path
        "uint8": (np.clip(np.round(128 + 70 * S), 0, 255).astype(np.uint8), 130.5),
        "int16": (np.round(9000 * S).astype(np.int16), 700.0),
        "float16": (S.astype(np.float16), 0.1),
    }
    return F


def _edge_ends(keys, shape):
    "lattice points q and q + d of edge ids"
    lin = (keys >> 3).astype(np.int64)
    d = (keys & 7).astype(np.int64)
    q = np.stack(np.unravel_index(lin, shape), axis=1)
    step = np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1)
    return q, q + step


def _gradient(A64):
    return np.stack(np.gradient(A64), axis=-1)      # numpy.gradient with its defaults: unit spacing, one-sided first difference on the rim


def _level1_edges(keys, S64, value):
    "low point, high point and ratio of every Level-1 vertex as cxp_k_vertices_f64 computes them"
    q, q1 = _edge_ends(keys, S64.shape)
    f0, f1 = S64[tuple(q.T)], S64[tuple(q1.T)]
    owner_low = ~(f0 > f1)
    flow, fhigh = np.where(owner_low, f0, f1), np.where(owner_low, f1, f0)
    den = 1.0 * (fhigh - flow)
    tiny = np.abs(den) <= 1e-8
    ratio = np.where(tiny, 0.5, (value - flow) / np.where(tiny, 1.0, den))
    a = np.where(owner_low[:, None], q, q1)
    b = np.where(owner_low[:, None], q1, q)
    return a, b, ratio, tiny, flow, fhigh


def _unit(g):
    n = np.linalg.norm(g, axis=1)
    return np.where(n[:, None] > 0, g / np.where(n > 0, n, 1.0)[:, None], 0.0), n


def _extract(A, value, generic=False):
    from contourist_amd import _ffi
    ctx = _ffi.Context()
    ctx.upload_grid_native(A)
    counts = ctx.extract3d(value, _ffi.CX_DIAG_CPYTHON310 | (_ffi.CX_KERNEL_GENERIC if generic else 0))
    assert counts["n_vertices"] > 0
    return ctx, counts


# ---- 1. Level 0 against float64 numpy, derived bound, no excluded vertices --------------------------------------------------
@pytest.mark.parametrize("name", ["sines", "noise", "ragged", "uint8", "int16", "float16"])
def test_level0_normals_against_numpy(name):
    """Every component of every vertex: |n_dev - n_ref| <= 32 * 2^-24 * (|G(a)|_1 + |G(b)|_1) / |g|, the fourth component to
    32 * 2^-24 * (|G(a)|_1 + |G(b)|_1).  A difference of two fp32 samples is one rounding; the lerp, the three squares, the
    reciprocal square root and the scaling add at most a dozen more; 32 is that count with a factor of two over it.  The
    reference is lerped with the DEVICE's fp32 fraction, so the fraction's own 1.5 ulp is not part of what is tested."""
    A, value = _fields()[name]
    ctx, counts = _extract(A, value)
    keys, t, _tris = ctx.download_level0_records(counts)
    N = ctx.level0_normals(counts)
    assert N.shape == (counts["n_vertices"], 4) and N.dtype == np.float32
    A64 = A.astype(np.float64)
    G = _gradient(A64)
    a, b = _edge_ends(keys, A.shape)
    Ga, Gb = G[tuple(a.T)], G[tuple(b.T)]
    g = Ga + t.astype(np.float64)[:, None] * (Gb - Ga)
    nref, length = _unit(g)
    bound = 32 * EPS32 * (np.abs(Ga).sum(axis=1) + np.abs(Gb).sum(axis=1))
    zero = length == 0
    assert np.all(N[zero] == 0)
    nz = ~zero
    err = np.abs(N[nz, :3].astype(np.float64) - nref[nz])
    print(name, "vertices", len(keys), "zero", int(zero.sum()), "worst err / bound", float((err / (bound[nz] / length[nz])[:, None]).max()),
          "worst |g| err / bound", float((np.abs(N[nz, 3] - length[nz]) / bound[nz]).max()))
    assert np.all(err <= (bound[nz] / length[nz])[:, None])
    assert np.all(np.abs(N[nz, 3].astype(np.float64) - length[nz]) <= bound[nz])
    ctx.close()


# ---- 2. Level 1 against float64 numpy ---------------------------------------------------------------------------------------
def _check_level1(ctx, post, S64, value, delta=None):
    keys = ctx.download_level1_keys(post)
    N = ctx.level1_normals(post, delta)
    a, b, ratio, _tiny, _lo, _hi = _level1_edges(keys, S64, value)
    G = _gradient(S64)
    g = G[tuple(a.T)] + ratio[:, None] * (G[tuple(b.T)] - G[tuple(a.T)])
    if delta is not None:
        g = g / np.asarray(delta, dtype=np.float64)
    nref, length = _unit(g)
    s = np.where((N * nref).sum(axis=1) < 0, -1.0, 1.0)
    err = np.abs(N - s[:, None] * nref)
    print("level 1 vertices", len(keys), "worst err", float(err.max()) if len(err) else 0.0, "flipped", int((s < 0).sum()))
    assert np.all(err <= 1e-12)
    return N, s, nref


@pytest.mark.parametrize("name", ["sines", "noise", "ragged", "uint8", "int16", "float16"])
def test_level1_normals_against_numpy(name):
    A, value = _fields()[name]
    ctx, counts = _extract(A, value)
    post = ctx.postprocess3d()
    A64 = A.astype(np.float64)
    _check_level1(ctx, post, A64, value)
    _check_level1(ctx, post, A64, value, delta=(0.5, 1.0, 2.0))      # the world normal: g / delta, renormalised
    ctx.close()


def test_level1_normals_callable_with_rim():
    "a sphere larger than its grid: the array carries a rim (origin -1) and float64 shadow samples"
    from numpy.linalg import norm
    from contourist_amd import tetrahedral
    S = tetrahedral.TriangulatedIsosurfaces((-1, -1, -1), (1, 1, 1), (0.25, 0.2, 0.33), lambda x, y, z: norm([x, y, z]), 1.3, [])
    S.search_for_endpoints()
    maker = S.contour_maker
    assert maker.grid_shift == 1 and maker.samples64 is not None
    points, _tris = S.get_points_and_triangles()
    ctx = maker.context()
    _check_level1(ctx, maker._post, np.asarray(maker.samples64, dtype=np.float64), 1.3)
    Nw, _s, _ = _check_level1(ctx, maker._post, np.asarray(maker.samples64, dtype=np.float64), 1.3, delta=S.grid.delta)
    assert np.array_equal(S.vertex_normals(), Nw) and len(Nw) == len(points)
    # the same callable as the second field: the isovalue at every vertex (float64 samples of g are rounded to fp32 on the way)
    vals = S.vertex_values(lambda x, y, z: norm([x, y, z]))
    assert vals.shape == (len(points),) and np.all(np.abs(vals - 1.3) <= 1e-6)


# ---- 3. sign, exactly -------------------------------------------------------------------------------------------------------
def _radial(n, fn):
    c = (n - 1) / 2.0
    I, J, K = np.meshgrid(*[np.arange(n, dtype=np.float64) - c] * 3, indexing="ij")
    return fn(np.sqrt(I * I + J * J + K * K)).astype(np.float32), c


def _signs(A, value):
    ctx, _counts = _extract(A, value)
    post = ctx.postprocess3d()
    _N, s, _ = _check_level1(ctx, post, A.astype(np.float64), value)
    pts, _t = ctx.download_level1(post)
    ctx.close()
    return s, pts, post


def test_sign_follows_the_orientation():
    "no tolerance, no excused vertices: a vertex whose normal disagrees with its component's winding fails"
    A, _c = _radial(33, lambda r: r * r)
    s, _pts, _post = _signs(A, 10.3 ** 2)
    assert np.all(s == 1.0)
    A, _c = _radial(33, lambda r: -(r * r))
    s, _pts, _post = _signs(A, -(10.3 ** 2))            # the reference orients outward, the gradient points inward
    assert np.all(s == -1.0)
    r1, r2 = 6.3, 12.6
    A, c = _radial(41, lambda r: -(r - r1) * (r - r2))
    s, pts, post = _signs(A, 0.0)
    assert post["n_components"] == 2
    radius = np.linalg.norm(pts - c, axis=1)
    inner = radius < 0.5 * (r1 + r2)
    assert inner.any() and (~inner).any()
    assert np.all(s[inner] == 1.0) and np.all(s[~inner] == -1.0)


# ---- 4. attributes ----------------------------------------------------------------------------------------------------------
def test_sampled_field_is_the_isovalue_and_the_coordinates():
    A, value = _fields()["sines"]
    ctx, counts = _extract(A, value)
    xyz, keys0, _t = ctx.download_level0(counts)
    # B = f: the isovalue, to the project's Level-0 tolerance 1e-6 |x| + 1e-6 (__graft_entry__.smoke)
    v0 = ctx.level0_sample(counts, A)
    print("level 0, B = f: worst", float(np.abs(v0 - value).max()))
    assert np.all(np.abs(v0.astype(np.float64) - value) <= 1e-6 * abs(value) + 1e-6)
    # B = the index grids: the coordinates
    idx = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in A.shape], indexing="ij")
    for axis in range(3):
        c0 = ctx.level0_sample(counts, idx[axis])
        assert np.all(np.abs(c0.astype(np.float64) - xyz[:, axis]) <= 1e-6 * np.abs(xyz[:, axis]) + 1e-6)
    # a random int16 grid against numpy: b1 - b0 is exact in fp32, the fused multiply-add rounds once (2^-24 relative); 2^-23 of the larger sample
    rng = np.random.default_rng(2)
    B = rng.integers(-30000, 30000, size=A.shape).astype(np.int16)
    keys, t, _t = ctx.download_level0_records(counts)
    a, b = _edge_ends(keys, A.shape)
    b0, b1 = B[tuple(a.T)].astype(np.float64), B[tuple(b.T)].astype(np.float64)
    got = ctx.level0_sample(counts, B).astype(np.float64)
    assert np.all(np.abs(got - (b0 + t.astype(np.float64) * (b1 - b0))) <= 2.0 ** -23 * np.maximum(1.0, np.maximum(np.abs(b0), np.abs(b1))))
    # ---- Level 1
    post = ctx.postprocess3d()
    k1 = ctx.download_level1_keys(post)
    A64 = A.astype(np.float64)
    la, lb, ratio, tiny, flow, fhigh = _level1_edges(k1, A64, value)
    v1 = ctx.level1_sample(post, A)
    expect = np.where(tiny, flow + 0.5 * (fhigh - flow), value)     # an edge that took the ratio = 0.5 rule is compared against that rule
    assert np.all(np.abs(v1 - expect) <= 1e-12 * np.maximum(1.0, np.abs(expect)))
    b0, b1 = B[tuple(la.T)].astype(np.float64), B[tuple(lb.T)].astype(np.float64)
    ref = b0 + ratio * (b1 - b0)
    assert np.all(np.abs(ctx.level1_sample(post, B) - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref)))
    ctx.close()


def test_level1_index_grids_are_the_coordinates():
    """B = the i, j, k index grids: the sampled values are the Level-1 points, compared before any tiny-collapse move, i.e. on
    the fixtures whose post-pass reports as many triangles after the tiny collapse as after the weld"""
    # (a tilted plane whose lattice values are multiples of 0.01, cut 0.003 away from them: no crossing comes near a lattice point)
    I, J, K = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in (24, 22, 26)], indexing="ij")
    plane = (I + 0.37 * J + 0.71 * K).astype(np.float32)
    candidates = [plane, plane, _radial(33, lambda r: r * r)[0], _fields()["sines"][0]]
    values = [10.123, 20.457, 10.3 ** 2, 0.1]
    checked = 0
    for A, value in zip(candidates, values):
        ctx, _counts = _extract(A, value)
        post = ctx.postprocess3d()
        if post["n_after_weld"] == post["n_after_tiny"]:
            checked += 1
            pts, _tr = ctx.download_level1(post)
            idx = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in A.shape], indexing="ij")
            for axis in range(3):
                c1 = ctx.level1_sample(post, idx[axis])
                assert np.all(np.abs(c1 - pts[:, axis]) <= 1e-12 * np.maximum(1.0, np.abs(pts[:, axis])))
        print("fixture", A.shape, value, "after weld", post["n_after_weld"], "after tiny", post["n_after_tiny"])
        ctx.close()
    assert checked > 0, "no fixture without a tiny-collapse move"


# ---- 5. plumbing ------------------------------------------------------------------------------------------------------------
def test_levels_select_repeat_and_invalidation():
    import ctypes
    from contourist_amd import _ffi
    A, _v = _fields()["sines"]
    values = [-0.3, 0.1, 0.45]
    ctx = _ffi.Context()
    ctx.upload_grid_native(A)
    single = _ffi.Context()
    single.upload_grid_native(A)
    all_counts = ctx.extract3d_levels(values)
    for i, v in enumerate(values):
        ctx.select_level(i)
        c1 = single.extract3d(v)
        n_lv, n_single = ctx.level0_normals(all_counts[i]), single.level0_normals(c1)
        assert n_lv.tobytes() == n_single.tobytes()                       # bit for bit
        assert ctx.level0_normals(all_counts[i]).tobytes() == n_lv.tobytes()    # two calls, the same bits
        p_lv, p_single = ctx.postprocess3d(), single.postprocess3d()
        m_lv = ctx.level1_normals(p_lv)
        assert m_lv.tobytes() == single.level1_normals(p_single).tobytes()
        assert ctx.level1_normals(p_lv).tobytes() == m_lv.tobytes()
    # a new extraction invalidates the Level-1 side, a new grid both: CX_ERR_INVALID, not stale data
    single.extract3d(0.2)
    out = ctypes.c_void_p()
    assert single.lib.cx_level1_normals(single.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    assert single.lib.cx_level1_sample_grid(single.handle, A.ctypes.data, 0, 0, ctypes.byref(out), None) == _ffi.CX_ERR_INVALID
    single.upload_grid_native(A)
    assert single.lib.cx_level0_normals(single.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    assert single.lib.cx_level0_sample_grid(single.handle, A.ctypes.data, 0, 0, ctypes.byref(out), None) == _ffi.CX_ERR_INVALID
    fresh = _ffi.Context()
    assert fresh.lib.cx_level0_normals(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    for c in (ctx, single, fresh):
        c.close()


def test_seeded_selection():
    "after a seeded selection Level 0 covers every vertex record, Level 1 what the selection kept"
    r1, r2 = 6.3, 12.6
    A, c = _radial(41, lambda r: -(r - r1) * (r - r2))
    ctx, counts = _extract(A, 0.0)
    mid = int(c)
    ctx.select_seeded([((mid, mid, mid), (mid, mid, mid + 8))])      # from the centre (f < 0) to between the spheres (f > 0): the inner sphere
    assert len(ctx.level0_normals(counts)) == counts["n_vertices"]
    post = ctx.postprocess3d()
    assert post["n_components"] == 1
    _N, s, _ = _check_level1(ctx, post, A.astype(np.float64), 0.0)
    assert len(s) == post["n_vertices"] and np.all(s == 1.0)
    ctx.close()


def test_unsupported_routes():
    from contourist_amd import tetrahedral
    d = 3.0 / 12
    S = tetrahedral.TriangulatedIsosurfaces([-1.5] * 3, [1.5 - d] * 3, [d] * 3, lambda x, y, z: x * x + y * y + z * z, 1.0, [], linear_interpolate=False)
    S.search_for_endpoints()
    S.get_points_and_triangles()
    with pytest.raises(NotImplementedError):
        S.vertex_normals()
    with pytest.raises(NotImplementedError):
        S.vertex_values(lambda x, y, z: x)
    ctx = S.contour_maker.context()
    with pytest.raises(NotImplementedError):                              # the C ABI's own answer after cx_postprocess3d_mesh
        ctx.level1_normals(S.contour_maker._post)
    with pytest.raises(NotImplementedError):
        ctx.write_level1(os.devnull, "ply_normals")
    # a volume marched in slabs (the limit lowered as the slab tests do)
    A, value = _fields()["sines"]
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    maker.MAX_SAMPLES_PER_EXTRACTION = 12 * A.shape[1] * A.shape[2]
    maker.get_points_and_triangles()
    with pytest.raises(NotImplementedError):
        maker.vertex_normals()
    with pytest.raises(NotImplementedError):
        maker.context().level1_normals(maker._post)
    # the sharded post-pass
    ctx2, _counts = _extract(A, value)
    ctx2.set_reference_corner(tuple(n - 1 for n in A.shape))
    ctx2.shard_begin(0, A.shape[0] - 1)
    sh = ctx2.shard_finish([], [])
    with pytest.raises(NotImplementedError):
        ctx2.level1_normals(sh)
    ctx2.close()


def test_device_tensors_and_python_api():
    torch = pytest.importorskip("torch")
    from contourist_amd import tetrahedral
    A, value = _fields()["int16"]
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    pts, _tris = maker.get_points_and_triangles()
    N = maker.vertex_normals()
    assert N.shape == (len(pts), 3) and N.dtype == np.float64
    Nd = maker.vertex_normals(device=True)
    assert Nd.is_cuda and np.array_equal(Nd.cpu().numpy(), N)
    B = torch.as_tensor(A.astype(np.float32)).cuda()
    V = maker.vertex_values(A)
    Vd = maker.vertex_values(B, device=True)
    assert Vd.is_cuda and np.array_equal(Vd.cpu().numpy(), V) and np.all(np.abs(V - value) <= 1e-12 * abs(value))
    N0 = maker.level0_normals()
    assert N0.shape == (len(maker.level0()["keys"]), 4)
    assert np.array_equal(maker.level0_normals(device=True).cpu().numpy(), N0)
    assert np.array_equal(maker.level0_values(B, device=True).cpu().numpy(), maker.level0_values(A))
    # several levels: the attributes of each level while it is current
    M = tetrahedral.MultiLevelIsosurfaces([0, 0, 0], None, [1, 1, 1], _fields()["sines"][0], [-0.3, 0.1])
    for level in M.levels():
        v, points, _triangles = level
        Nl = level.vertex_normals()
        single = tetrahedral.TriangulatedIsosurfaces([0, 0, 0], None, [1, 1, 1], _fields()["sines"][0], v, [])
        single.search_for_endpoints()
        assert np.array_equal(np.asarray(single.get_points_and_triangles()[0]), np.asarray(points))
        assert np.array_equal(single.vertex_normals(), Nl)


# ---- 6. files ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32", "noise24_v0"])
def test_files_with_normals(name, tmp_path):
    from contourist_amd import tetrahedral, mesh_io
    G = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    S = tetrahedral.TriangulatedIsosurfaces(G["mins"], None, G["delta"], G["A"], float(G["value"]), [])
    S.search_for_endpoints()
    before_ply, before_gltf = str(tmp_path / "before.ply"), str(tmp_path / "before.gltf")
    mesh_io.write_ply_device(S, before_ply)
    mesh_io.write_gltf_device(S, before_gltf)
    p_dev = str(tmp_path / "device_n.ply")
    info = mesh_io.write_ply_device(S, p_dev, normals=True)
    ctx = S.contour_maker.context()
    pts_grid, tris_dev = ctx.download_level1(S.contour_maker._post)
    world = S.grid.from_grid_coordinates(pts_grid)
    N = S.vertex_normals()
    p_host = str(tmp_path / "host_n.ply")
    mesh_io.write_ply(p_host, world, tris_dev, normals=N)
    assert open(p_dev, "rb").read() == open(p_host, "rb").read()
    assert info["n_vertices"] == len(world) and info["bytes"] == os.path.getsize(p_dev)
    assert np.array_equal(info["min"], world.min(axis=0)) and np.array_equal(info["max"], world.max(axis=0))
    P, T, Nr = mesh_io.read_ply(p_dev, normals=True)
    assert np.array_equal(P, world) and np.array_equal(T, tris_dev) and np.array_equal(Nr, N)
    # glTF: three sections at the offsets the JSON names
    g_dev = str(tmp_path / "device_n.gltf")
    mesh_io.write_gltf_device(S, g_dev, normals=True)
    doc = json.load(open(g_dev))
    blob = open(str(tmp_path / "device_n.bin"), "rb").read()
    nv, nt = len(world), len(tris_dev)
    assert doc["buffers"][0]["byteLength"] == len(blob) == nv * 24 + nt * 12
    prim = doc["meshes"][0]["primitives"][0]
    views, acc = doc["bufferViews"], doc["accessors"]

    def section(accessor, dtype, width):
        v = views[acc[accessor]["bufferView"]]
        return np.frombuffer(blob[v["byteOffset"]:v["byteOffset"] + v["byteLength"]], dtype=dtype).reshape(-1, width)
    pos, nrm, idx = section(prim["attributes"]["POSITION"], "<f4", 3), section(prim["attributes"]["NORMAL"], "<f4", 3), section(prim["indices"], "<u4", 3)
    assert acc[prim["attributes"]["NORMAL"]] == {"bufferView": 2, "componentType": 5126, "count": nv, "type": "VEC3"}
    assert np.array_equal(pos, world.astype(np.float32)) and np.array_equal(idx, tris_dev.astype(np.uint32))
    assert np.array_equal(nrm, N.astype(np.float32))
    assert np.all(np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1.0) <= 1e-6)
    # formats 0 and 1 keep their bytes, before and after the normals were asked for
    after_ply, after_gltf = str(tmp_path / "after.ply"), str(tmp_path / "after.gltf")
    mesh_io.write_ply_device(S, after_ply)
    mesh_io.write_gltf_device(S, after_gltf)
    assert open(before_ply, "rb").read() == open(after_ply, "rb").read()
    assert open(str(tmp_path / "before.bin"), "rb").read() == open(str(tmp_path / "after.bin"), "rb").read()
    assert json.load(open(before_gltf))["accessors"] == json.load(open(after_gltf))["accessors"]
