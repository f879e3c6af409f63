"""Mean, Gaussian and principal curvature at the vertices (cx_attr.hip), Level 0 and Level 1, against the float64
numpy restatement tests/curvature_ref.py of the definition in include/contourist_hip.h ("vertex attributes")."""
import ctypes

import numpy as np
import pytest

import curvature_ref as cr

pytestmark = pytest.mark.gpu

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
C32, C64 = 16, 32


def _sines(shape=(40, 36, 44), seed=3):
    rng = np.random.default_rng(seed)
    g0, g1, g2 = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
    return (np.sin(3.1 * g0 + 0.4) * np.cos(2.7 * g1) + 0.8 * np.sin(3.9 * g2 + 1.0) + 0.05 * rng.standard_normal(shape)).astype(np.float32)


def _fields():
    "name -> (sample array in its own type, isovalue): the fields of tests/test_gpu_normals.py"
    rng = np.random.default_rng(11)
    S = _sines()
    return {
        "sines": (S, 0.1),
        "noise": (rng.standard_normal((28, 30, 32)).astype(np.float32), 0.1),
        "ragged": (_sines((9, 7, 3), seed=5), 0.1),                      # the smallest legal shape: every wave is on the rim path
        "uint8": (np.clip(np.round(128 + 70 * S), 0, 255).astype(np.uint8), 130.5),
        "int16": (np.round(9000 * S).astype(np.int16), 700.0),
        "float16": (S.astype(np.float16), 0.1),
    }


def _radial(n, fn):
    c = (n - 1) / 2.0
    I, J, K = np.meshgrid(*[np.arange(n, dtype=np.float64) - c] * 3, indexing="ij")
    return fn(np.sqrt(I * I + J * J + K * K)).astype(np.float32), c


def _edge_ends(keys, shape):
    "lattice points q and q + d of edge ids"
    lin = (keys >> 3).astype(np.int64)
    d = (keys & 7).astype(np.int64)
    q = np.stack(np.unravel_index(lin, shape), axis=1)
    step = np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1)
    return q, q + step


def _level1_edges(keys, S64, value):
    "low point, high point and ratio of every Level-1 vertex as cxp_k_vertices_f64 computes them"
    q, q1 = _edge_ends(keys, S64.shape)
    f0, f1 = S64[tuple(q.T)], S64[tuple(q1.T)]
    owner_low = ~(f0 > f1)
    flow, fhigh = np.where(owner_low, f0, f1), np.where(owner_low, f1, f0)
    den = 1.0 * (fhigh - flow)
    tiny = np.abs(den) <= 1e-8
    ratio = np.where(tiny, 0.5, (value - flow) / np.where(tiny, 1.0, den))
    return np.where(owner_low[:, None], q, q1), np.where(owner_low[:, None], q1, q), ratio


def _extract(A, value, generic=False):
    from contourist_amd import _ffi
    ctx = _ffi.Context()
    ctx.upload_grid_native(A)
    counts = ctx.extract3d(value, _ffi.CX_DIAG_CPYTHON310 | (_ffi.CX_KERNEL_GENERIC if generic else 0))
    assert counts["n_vertices"] > 0
    return ctx, counts


def _ratio(err, bound):
    "worst err / bound over the rows with a positive bound (0 when there are none)"
    ok = bound > 0
    return float((err[ok] / bound[ok]).max()) if ok.any() else 0.0


def _assert_within(label, got, ref, eps, C, sign=None):
    """the three bounds of the issue on every row, none excluded; rows with |g| == 0 must be four zeros.  sign (+-1 per row): what
    the orientation did to the vertex -- mean, k1, k2 carry it (k1 and k2 swap), gauss does not."""
    bm, bk, bp = cr.bounds(ref, eps, C)
    s = np.ones(len(got)) if sign is None else sign
    want = np.stack([s * ref["mean"], ref["gauss"], np.where(s > 0, ref["k1"], -ref["k2"]), np.where(s > 0, ref["k2"], -ref["k1"])], axis=1)
    err = np.abs(got.astype(np.float64) - want)
    zero = ref["g"] == 0
    print(label, "vertices", len(got), "zero", int(zero.sum()), "worst err / bound: mean", _ratio(err[:, 0], bm), "gauss", _ratio(err[:, 1], bk),
          "k1", _ratio(err[:, 2], bp), "k2", _ratio(err[:, 3], bp))
    assert np.all(got[zero] == 0)
    assert np.all(err[:, 0] <= bm), label + ": mean"
    assert np.all(err[:, 1] <= bk), label + ": gauss"
    assert np.all(err[:, 2] <= bp) and np.all(err[:, 3] <= bp), label + ": k1, k2"
    assert np.all(got[:, 2] >= got[:, 3]), label + ": k1 >= k2"


# ---- 1. Level 0 against the reference, every vertex ---------------------------------------------------------------------------
def _check_level0(name, delta=None, generic=False):
    A, value = _fields()[name]
    ctx, counts = _extract(A, value, generic)
    keys, t, _tris = ctx.download_level0_records(counts)
    K = ctx.level0_curvature(counts, delta)
    assert K.shape == (counts["n_vertices"], 4) and K.dtype == np.float32
    a, b = _edge_ends(keys, A.shape)
    ref = cr.curvature(A.astype(np.float64), a, b, t.astype(np.float64), delta)      # lerped with the DEVICE's fp32 fraction
    _assert_within("level 0 %s delta=%s generic=%s" % (name, delta, generic), K, ref, EPS32, C32)
    ctx.close()


@pytest.mark.parametrize("name", ["sines", "noise", "ragged", "uint8", "int16", "float16"])
def test_level0_curvature_against_numpy(name):
    """|mean - ref| <= bm = C eps (D/|g|)(Gs/|g|), |gauss - ref| <= bk = C eps (D/|g|)^2 (Gs/|g|), |k - ref| <= bm + sqrt(2|mean| bm +
    bm^2 + bk) with eps = 2^-24 and C = 16: every fp32 difference of two samples is one rounding relative to its result, the lerps,
    the normalisation and the quadratic forms add about a dozen more.  Every vertex, none excluded."""
    _check_level0(name)


def test_level0_curvature_world_spacing():
    _check_level0("sines", delta=(0.5, 1.0, 2.0))


def test_level0_curvature_generic_kernels():
    _check_level0("noise", generic=True)


# ---- 2. Level 1 against the reference -----------------------------------------------------------------------------------------
def _check_level1(label, ctx, post, S64, value, delta=None):
    keys = ctx.download_level1_keys(post)
    K = ctx.level1_curvature(post, delta)
    N = ctx.level1_normals(post, delta)
    assert K.shape == (post["n_vertices"], 4) and K.dtype == np.float64
    a, b, ratio = _level1_edges(keys, S64, value)
    ref = cr.curvature(S64, a, b, ratio, delta)
    sign = np.where((N * ref["n"]).sum(axis=1) < 0, -1.0, 1.0)         # what vertex_normals() of the same mesh says
    _assert_within("level 1 %s delta=%s flipped=%d" % (label, delta, int((sign < 0).sum())), K, ref, EPS64, C64, sign)
    return K, sign


@pytest.mark.parametrize("name", ["sines", "noise", "ragged", "uint8", "int16", "float16"])
def test_level1_curvature_against_numpy(name):
    "the same three bounds with eps = 2^-53 and C = 32 (both sides round), with and without a world spacing"
    A, value = _fields()[name]
    ctx, _counts = _extract(A, value)
    post = ctx.postprocess3d()
    A64 = A.astype(np.float64)
    _check_level1(name, ctx, post, A64, value)
    _check_level1(name, ctx, post, A64, value, delta=(0.5, 1.0, 2.0))
    ctx.close()


def test_level1_sign_follows_the_orientation():
    """two concentric spheres of one field: the inner one keeps the gradient's side, the outer one is reversed.  Both are wound
    outwards, so after the sign both are convex: mean > 0 and k1 >= k2 > 0 everywhere, gauss > 0 untouched"""
    r1, r2 = 6.3, 12.6
    A, c = _radial(41, lambda r: -(r - r1) * (r - r2))
    ctx, _counts = _extract(A, 0.0)
    post = ctx.postprocess3d()
    assert post["n_components"] == 2
    K, sign = _check_level1("two shells", ctx, post, A.astype(np.float64), 0.0)
    pts, _t = ctx.download_level1(post)
    inner = np.linalg.norm(pts - c, axis=1) < 0.5 * (r1 + r2)
    assert inner.any() and (~inner).any()
    assert np.all(sign[inner] == 1.0) and np.all(sign[~inner] == -1.0)
    assert np.all(K[:, 0] > 0) and np.all(K[:, 1] > 0) and np.all(K[:, 3] > 0)
    ctx.close()
    # one sphere whose field grows inwards: every vertex reversed
    A, _c = _radial(33, lambda r: -(r * r))
    ctx, _counts = _extract(A, -(10.3 ** 2))
    post = ctx.postprocess3d()
    K, sign = _check_level1("inward sphere", ctx, post, A.astype(np.float64), -(10.3 ** 2))
    assert np.all(sign == -1.0) and np.all(K[:, 0] > 0)
    ctx.close()


# ---- 3. Gauss-Bonnet across subsystems: curvature, the downloaded mesh, the components and topology() --------------------------
@pytest.mark.parametrize("name", ["sphere", "two_spheres", "torus", "double_torus"])
def test_gauss_bonnet(name):
    """per component, sum(gauss * vertex area) / 2 pi lies within 0.5 of the Euler number topology() reports (integrality, not a
    measurement; tests/test_curvature_host.py confirms that the reference alone stays within it on these fields)"""
    from contourist_amd import tetrahedral
    A, eulers = cr.gauss_bonnet_fields()[name]
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, 0.0)
    pts, tris = maker.get_points_and_triangles()
    K = maker.vertex_curvature()
    topo = maker.topology()
    _tl, vl = maker.component_labels()
    assert len(K) == len(pts) == len(vl) and sorted(int(e) for e in topo["euler"]) == sorted(eulers)
    area = cr.vertex_areas(pts, tris)
    for c in range(len(topo)):
        total = float((K[vl == c, 1] * area[vl == c]).sum() / (2 * np.pi))
        print(name, "component", c, "vertices", int((vl == c).sum()), "Euler number", int(topo["euler"][c]), "integral / 2 pi", total)
        assert abs(total - int(topo["euler"][c])) < 0.5
    if name == "sphere":
        worst = float(np.abs(K[:, 0] * 9.3 - 1).max())
        print("sphere: worst relative error of mean against 1/R", worst)
        assert worst <= cr.SPHERE_MEAN_RTOL


# ---- 4. API routes ------------------------------------------------------------------------------------------------------------
def test_api_routes_agree():
    torch = pytest.importorskip("torch")
    from contourist_amd import tetrahedral
    A, value = _fields()["sines"]
    delta = [0.5, 1.0, 2.0]
    S = tetrahedral.TriangulatedIsosurfaces([0, 0, 0], None, delta, A, value, [])
    S.search_for_endpoints()
    pts, _tris = S.get_points_and_triangles()
    Kw = S.vertex_curvature()
    assert Kw.shape == (len(pts), 4) and Kw.dtype == np.float64
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    assert np.array_equal(maker.vertex_curvature(delta=delta), Kw)
    Kd = maker.vertex_curvature(device=True)
    assert Kd.is_cuda and Kd.dtype == torch.float64 and np.array_equal(Kd.cpu().numpy(), maker.vertex_curvature())
    K0 = maker.level0_curvature()
    assert K0.shape == (len(maker.level0()["keys"]), 4) and K0.dtype == np.float32
    K0d = maker.level0_curvature(device=True)
    assert K0d.is_cuda and K0d.dtype == torch.float32 and np.array_equal(K0d.cpu().numpy(), K0)
    # several levels: the curvature of each level while it is current
    values = [-0.3, 0.1]
    M = tetrahedral.MultiLevelIsosurfaces([0, 0, 0], None, delta, A, values)
    seen = 0
    for level in M.levels():
        v, points, _triangles = level
        Kl = level.vertex_curvature()
        single = tetrahedral.TriangulatedIsosurfaces([0, 0, 0], None, delta, A, v, [])
        single.search_for_endpoints()
        assert np.array_equal(np.asarray(single.get_points_and_triangles()[0]), np.asarray(points))
        assert np.array_equal(single.vertex_curvature(), Kl)
        seen += 1
    assert seen == len(values)


def test_filtered_mesh_repeat_and_normals():
    A, _eulers = cr.gauss_bonnet_fields()["two_spheres"]
    ctx, counts = _extract(A, 0.0)
    post = ctx.postprocess3d()
    assert post["n_components"] == 2
    # two calls in a row, and the normals before and after: the same bits everywhere
    K = ctx.level1_curvature(post)
    assert ctx.level1_curvature(post).tobytes() == K.tobytes()
    N = ctx.level1_normals(post)
    assert ctx.level1_curvature(post).tobytes() == K.tobytes()
    assert ctx.level1_normals(post).tobytes() == N.tobytes()
    K0 = ctx.level0_curvature(counts)
    N0 = ctx.level0_normals(counts)
    assert ctx.level0_curvature(counts).tobytes() == K0.tobytes() and ctx.level0_normals(counts).tobytes() == N0.tobytes()
    # the filtered mesh: its own length, the rows of the vertices that stayed (matched by their edge ids)
    keys = ctx.download_level1_keys(post)
    table = ctx.level1_components()
    keep = np.zeros(len(table), dtype=bool)
    keep[int(np.argmax(table["triangles"]))] = True
    kept = ctx.level1_keep_components(keep)
    assert 0 < kept["n_vertices"] < post["n_vertices"]
    Kf = ctx.level1_curvature(kept)
    keys_f = ctx.download_level1_keys(kept)
    assert Kf.shape == (kept["n_vertices"], 4)
    order = np.argsort(keys)
    rows = order[np.searchsorted(keys[order], keys_f)]
    assert np.array_equal(keys[rows], keys_f) and Kf.tobytes() == K[rows].tobytes()
    ctx.close()


def test_keep_components_through_the_python_api():
    from contourist_amd import tetrahedral
    A, _eulers = cr.gauss_bonnet_fields()["two_spheres"]
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, 0.0)
    maker.get_points_and_triangles()
    before = maker.vertex_curvature()
    counts = maker.keep_components(largest=1)
    after = maker.vertex_curvature()
    pts, _tris = maker.get_points_and_triangles()
    assert len(after) == counts["n_vertices"] == len(pts) < len(before)


# ---- 5. refusals, each with its error code --------------------------------------------------------------------------------------
def test_refusals():
    from contourist_amd import _ffi, tetrahedral
    out = ctypes.c_void_p()
    # before any extraction
    fresh = _ffi.Context()
    assert fresh.lib.cx_level0_curvature(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    assert fresh.lib.cx_level1_curvature(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    A, value = _fields()["sines"]
    fresh.upload_grid_native(A)
    assert fresh.lib.cx_level0_curvature(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    counts = fresh.extract3d(value)
    assert fresh.lib.cx_level1_curvature(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID     # no post-pass yet
    bad = np.array([1.0, 0.0, 1.0])
    assert fresh.lib.cx_level0_curvature(fresh.handle, bad.ctypes.data, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    # a next extraction invalidates Level 1, as for the normals
    post = fresh.postprocess3d()
    assert len(fresh.level1_curvature(post)) == post["n_vertices"]
    fresh.extract3d(0.2)
    assert fresh.lib.cx_level1_curvature(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    assert fresh.lib.cx_level1_normals(fresh.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_INVALID
    fresh.close()
    # an axis shorter than 3 samples
    thin = _sines((6, 5, 2), seed=7)
    ctx, counts = _extract(thin, 0.1)
    assert ctx.lib.cx_level0_curvature(ctx.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_UNSUPPORTED
    assert b"3 samples" in ctx.lib.cx_last_error(ctx.handle)
    with pytest.raises(NotImplementedError):
        ctx.level0_curvature(counts)
    post = ctx.postprocess3d()
    assert ctx.lib.cx_level1_curvature(ctx.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        ctx.level1_curvature(post)
    ctx.close()
    # after simplify(): the vertices are cluster means, and the message says so
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    maker.get_points_and_triangles()
    assert len(maker.vertex_curvature()) > 0
    maker.simplify(cell=2.0)
    mctx = maker.context()
    assert mctx.lib.cx_level1_curvature(mctx.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_UNSUPPORTED
    assert b"cluster means" in mctx.lib.cx_last_error(mctx.handle)
    with pytest.raises(NotImplementedError):
        maker.vertex_curvature()
    assert len(maker.level0_curvature()) == len(maker.level0()["keys"])       # Level 0 is still the extraction's
    # after cx_postprocess3d_mesh (refined points)
    d = 3.0 / 12
    S = tetrahedral.TriangulatedIsosurfaces([-1.5] * 3, [1.5 - d] * 3, [d] * 3, lambda x, y, z: x * x + y * y + z * z, 1.0, [], linear_interpolate=False)
    S.search_for_endpoints()
    S.get_points_and_triangles()
    with pytest.raises(NotImplementedError):
        S.vertex_curvature()
    sctx = S.contour_maker.context()
    assert sctx.lib.cx_level1_curvature(sctx.handle, None, ctypes.byref(out)) == _ffi.CX_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        sctx.level1_curvature(S.contour_maker._post)
