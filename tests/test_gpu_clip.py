"""Clipping of the Level-1 mesh on the device (cx_clip.hip) against tests/clip_ref.py, the numpy restatement of the header's section
"clipping", run on the mesh downloaded BEFORE the call (points, triangles in device order, normals).  The orientation step only
reverses whole components: rows are compared after undoing the reversal the components' `flipped` reports.

With clean, the comparison is against oracle.postpass.clean on the restatement's raw lists.  The share of triangles whose cross
product the reference's np.allclose area rule sits on the edge of is computed on the host with the operands of the cross product
swapped (the oracle against itself); every case prints it and asserts that it is 0.0, so no triangle is excluded from a comparison.

Carried normals (test_normals): the interpolation and the normalisation round on the device as numpy rounds them (contraction off,
IEEE square root and division); the test prints the largest difference to the restatement in ulps (0.0) and asserts equal bytes."""
import numpy as np
import pytest

import clip_ref as R
import topology_ref

pytestmark = pytest.mark.gpu

SPHERE_C = (23.3, 22.6, 24.2)
OBLIQUE = ((0.36, 0.48, 0.8), 0.36 * 23.3 + 0.48 * 22.6 + 0.8 * 24.2 + 1.37)
PLANES = [OBLIQUE, ((1.0, 0.0, 0.0), 24.0), ((1.0, 0.0, 0.0), 23.5), ((1.0, 0.0, 0.0), -5.0)]          # the last one misses every mesh here
SMALL_PLANES = [((0.36, 0.48, 0.8), 0.36 * 3.3 + 0.48 * 3.6 + 0.8 * 4.2 + 0.2), ((1.0, 0.0, 0.0), 3.0), ((1.0, 0.0, 0.0), 3.5), ((1.0, 0.0, 0.0), -5.0)]


def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def _ball(shape, c, r):
    I, J, K = _grid(shape)
    return np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2) - r


def _field(name):
    if name == "sphere":
        return _ball((48, 48, 48), SPHERE_C, 15.4).astype(np.float32), 0.0
    if name == "two_blobs":
        return np.minimum(_ball((48, 40, 40), (13.2, 19.4, 20.1), 9.3), _ball((48, 40, 40), (34.3, 20.6, 18.9), 7.1)).astype(np.float32), 0.0
    if name == "torus":
        I, J, K = _grid((48, 48, 32))
        return (np.sqrt((np.sqrt((I - 23.4) ** 2 + (J - 23.7) ** 2) - 13.2) ** 2 + (K - 15.3) ** 2) - 5.1).astype(np.float32), 0.0
    if name == "noise":
        from contourist_amd import synthetic
        return synthetic.smooth_noise_host((96, 96, 96), 7, 6).astype(np.float32), 0.8
    if name == "two_blobs_u8":
        A, _v = _field("two_blobs")
        return np.clip(np.round(128.0 + 8.0 * A.astype(np.float64)), 0, 255).astype(np.uint8), 128.5
    if name == "octahedron":          # fewer than 64 triangles: a partial wave
        I, J, K = _grid((8, 8, 8))
        return (abs(I - 3.3) + abs(J - 3.6) + abs(K - 4.2) - 1.0).astype(np.float32), 0.0
    if name == "empty":
        return _field("octahedron")[0], 1.0e9
    raise KeyError(name)


def _context(A, value):
    from contourist_amd import _ffi
    ctx = _ffi.Context()
    ctx.upload_grid_native(A)
    ctx.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    return ctx, ctx.postprocess3d()


def _after(ctx, out):
    p2, t2 = ctx.download_level1(out)
    table = ctx.level1_components()
    tl2, _vl2 = ctx.level1_component_labels()
    lo_hi, t = ctx.level1_clip_map()
    return dict(points=p2, triangles=t2, rows=R.unflip(t2, tl2, table["flipped"]), keys=ctx.download_level1_keys(out), lo_hi=lo_hi, t=t, table=table, tl=tl2)


def _flags(below=False, clean=False, normals=False):
    from contourist_amd import _ffi
    return (0 if clean else _ffi.CX_CLIP_NO_CLEAN) | (_ffi.CX_CLIP_KEEP_BELOW if below else 0) | (_ffi.CX_CLIP_NORMALS if normals else 0)


def _compare(out, ref, G, what):
    "every count and every array of a CX_CLIP_NO_CLEAN result against the restatement"
    for k in ("n_cut_vertices", "n_cut_triangles", "n_nonfinite", "n_on_cut"):
        assert out[k] == ref[k], (what, k, out[k], ref[k])
    assert out["n_raw_triangles"] == len(ref["raw_triangles"]), what
    assert out["n_vertices"] == len(ref["points"]) and out["n_triangles"] == len(ref["triangles"]), (what, out)
    assert out["n_components"] == len(G["table"]), what
    assert G["points"].tobytes() == ref["points"].tobytes(), what
    assert np.array_equal(G["rows"], ref["triangles"]), what
    assert np.array_equal(G["keys"], ref["keys"]), what
    assert np.array_equal(G["lo_hi"], ref["map_lo_hi"]) and G["t"].tobytes() == ref["map_t"].tobytes(), what


# ---- 1. exact parity without clean -------------------------------------------------------------------------------------------
_FIELDS = ["sphere", "two_blobs", "torus", "noise", "two_blobs_u8", "octahedron", "empty"]
_shared = {}


@pytest.fixture(scope="module")
def parity_context():
    "one context per field for the cases of the parity test (the 96^3 noise field is generated and marched once)"
    def get(name):
        if name not in _shared:
            A, value = _field(name)
            _shared[name] = _context(A, value)
        return _shared[name]
    yield get
    for ctx, _post in _shared.values():
        ctx.close()
    _shared.clear()


@pytest.mark.parametrize("plane", range(4), ids=["oblique", "through_vertices", "between_vertices", "misses"])
@pytest.mark.parametrize("name", _FIELDS)
def test_exact_parity_without_clean(name, plane, parity_context):
    ctx, post = parity_context(name)
    if name == "octahedron":
        assert 0 < post["n_triangles"] < 64
    if name == "empty":
        assert post["n_triangles"] == 0
    normal, offset = (SMALL_PLANES if name in ("octahedron", "empty") else PLANES)[plane]
    for below in (False, True):
        what = "%s plane %s %s below=%s" % (name, normal, offset, below)
        post = ctx.postprocess3d()
        pts, tris = ctx.download_level1(post)
        ref = R.clip(pts, tris, R.plane_scalars(pts, normal), offset, keep_below=below)
        out = ctx.level1_clip_plane(normal, offset, _flags(below))
        G = _after(ctx, out)
        print(what, "->", out)
        _compare(out, ref, G, what)
        if offset == -5.0 and not below:            # all kept: the mesh is the source
            assert G["points"].tobytes() == pts.tobytes() and G["triangles"].tobytes() == tris.tobytes(), what
            assert out["n_cut_vertices"] == 0 and np.array_equal(G["lo_hi"][:, 0], np.arange(len(pts)))
        if offset == -5.0 and below:                # all dropped: an empty mesh, no error
            assert out["n_vertices"] == 0 and out["n_triangles"] == 0 and out["n_components"] == 0, what
        if name == "sphere" and plane == 1:
            assert out["n_on_cut"] == 208 and out["n_cut_vertices"] == 3            # the d == 0 rule at work (worked out on the host beforehand)


# ---- 2. with clean -----------------------------------------------------------------------------------------------------------
def _edge_share(P, T):
    "share of triangles the np.allclose area rule decides differently with the operands of the cross product swapped"
    A, B, C = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    d1 = np.all(np.abs(np.cross(A - C, B - C)) <= 1e-8, axis=1)
    d2 = np.all(np.abs(np.cross(B - C, A - C)) <= 1e-8, axis=1)
    return float(np.count_nonzero(d1 != d2)) / max(1, len(T))


def _check_clean(ctx, ref, out, what):
    from oracle import postpass
    G = _after(ctx, out)
    share = _edge_share(ref["raw_points"], ref["raw_triangles"])
    print(what, "share of triangles on the edge of the area rule:", share, "raw", len(ref["raw_triangles"]), "->", out["n_triangles"])
    assert share == 0.0      # (no triangle sits on the edge of the rule: nothing is excluded below)
    src = ref["raw_source"]
    x2, t2 = postpass.clean(ref["raw_points"], ref["raw_triangles"], np.stack([src, src, src], axis=1))
    want = set(map(tuple, np.asarray(t2).tolist()))
    got = set(map(tuple, G["rows"].tolist()))
    assert G["points"].tobytes() == np.asarray(x2).tobytes() and got == want, (what, len(got ^ want))
    assert out["n_cut_vertices"] == ref["n_cut_vertices"] and out["n_raw_triangles"] == len(ref["raw_triangles"]) >= out["n_triangles"]
    return G, t2


@pytest.mark.parametrize("name", ["sphere", "two_blobs", "torus"])
def test_with_clean_against_the_oracle(name):
    A, value = _field(name)
    ctx, post = _context(A, value)
    try:
        for normal, offset in PLANES[:3]:
            for below in (False, True):
                post = ctx.postprocess3d()
                pts, tris = ctx.download_level1(post)
                ref = R.clip(pts, tris, R.plane_scalars(pts, normal), offset, keep_below=below)
                out = ctx.level1_clip_plane(normal, offset, _flags(below, clean=True))
                _check_clean(ctx, ref, out, "%s plane %s %s below=%s" % (name, normal, offset, below))
    finally:
        ctx.close()


def test_clean_has_work():
    """the sphere and the oblique plane, the scalars of the 16 inside and the 16 outside vertices nearest the plane set to +-1e-13: cut
    vertices land within 1e-13 of those vertices, 92 raw triangles are degenerate, the clean rule merges and drops"""
    A, value = _field("sphere")
    ctx, post = _context(A, value)
    try:
        pts, tris = ctx.download_level1(post)
        s = R.plane_scalars(pts, OBLIQUE[0]) - OBLIQUE[1]
        ins, outs = np.nonzero(s >= 0)[0], np.nonzero(s < 0)[0]
        s[ins[np.argsort(s[ins], kind="stable")[:16]]] = 1e-13
        s[outs[np.argsort(-s[outs], kind="stable")[:16]]] = -1e-13
        ref = R.clip(pts, tris, s, 0.0)
        out = ctx.level1_clip_scalars(s, 0.0, _flags(clean=True))
        G, t2 = _check_clean(ctx, ref, out, "sphere, nudged scalars")
        assert len(ref["raw_triangles"]) == 12851 and out["n_triangles"] == 12759 == len(t2)
        topo = ctx.level1_topology()
        assert len(topo) == 1 and topo["euler"][0] == 1
    finally:
        ctx.close()


# ---- 3. topology of the result -----------------------------------------------------------------------------------------------
def _topology(ctx, out, what):
    _pts, tris = ctx.download_level1(out)
    tl, _vl = ctx.level1_component_labels()
    want = topology_ref.topology(tris, tl)
    table = ctx.level1_topology()
    loops, verts = ctx.level1_boundary_loops()
    assert table.tobytes() == want[0].tobytes() and loops.tobytes() == want[1].tobytes() and np.array_equal(verts, want[2]), what
    return table, loops, verts


def _d_bound(normal, offset):
    """|n.p - offset| of a vertex ON the cut, evaluated in float64, with u = 2^-53 and M = (|n0| + |n1| + |n2|) * 64 + |offset| (the
    coordinates are below 64): d[lo], d[hi] are each off by at most 4 u M (three products, two sums, one difference); the exact point at
    the computed t has a plane value of at most that; the computed point is off per coordinate by at most (5 |p_hi - p_lo| + 64) u <= 74 u
    (edge length below 2), that is 1.2 u M on the plane value; evaluating the plane again costs 4 u M: 9.2 u M in all, 10 u M asserted.
    A vertex with d == 0 is on the cut exactly.  Nothing here is measured."""
    M = float(np.sum(np.abs(normal))) * 64.0 + abs(offset)
    return 10.0 * 2.0 ** -53 * M


@pytest.mark.parametrize("clean", [True, False])
def test_topology_of_the_result(clean):
    sphere, torus = _field("sphere")[0], _field("torus")[0]
    cases = [("sphere", sphere, OBLIQUE, False, (1, 1, 0)), ("sphere", sphere, OBLIQUE, True, (1, 1, 0)), ("sphere", sphere, PLANES[1], False, (1, 1, 0)),
             ("torus", torus, OBLIQUE, False, (1, 1, 0)), ("torus", torus, OBLIQUE, True, (-1, 1, 1)),
             ("torus", torus, PLANES[2], False, (0, 2, 0)), ("torus", torus, PLANES[2], True, (0, 2, 0)),
             ("torus", torus, ((0.0, 0.0, 1.0), 15.3), False, (0, 2, 0)), ("torus", torus, ((0.0, 0.0, 1.0), 15.3), True, (0, 2, 0))]
    ctxs = {}
    try:
        for name, A, (normal, offset), below, (euler, nloops, genus) in cases:
            if name not in ctxs:
                ctxs[name] = _context(A, 0.0)[0]
            ctx = ctxs[name]
            post = ctx.postprocess3d()
            src = ctx.level1_topology()
            assert len(src) == 1 and src["boundary_edges"][0] == 0          # a closed source: every boundary of the result is the cut
            out = ctx.level1_clip_plane(normal, offset, _flags(below, clean=clean))
            what = "%s %s %s below=%s clean=%s" % (name, normal, offset, below, clean)
            table, loops, verts = _topology(ctx, out, what)
            print(what, "euler", table["euler"].tolist(), "loops", table["boundary_loops"].tolist(), "genus", table["genus"].tolist())
            assert len(table) == 1 and (table["euler"][0], table["boundary_loops"][0], table["genus"][0]) == (euler, nloops, genus), what
            assert np.all(loops["simple"] == 1), what
            if not clean:       # (the clean rule may merge a cut vertex into an old vertex 1e-8 away: the bound is the interpolation's alone)
                P = ctx.download_level1(out)[0]
                d = np.abs(R.plane_scalars(P[verts], normal) - offset)
                print(what, "largest |d| on the cut curve", float(d.max()), "bound", _d_bound(normal, offset))
                assert float(d.max()) <= _d_bound(normal, offset), what
    finally:
        for ctx in ctxs.values():
            ctx.close()


# ---- 4. area -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere", "torus", "two_blobs"])
def test_the_two_sides_add_up_to_the_source(name):
    """cut points are rounded to an ulp of a coordinate below 64 (7e-15) on at most ~3e4 triangles of edge length below 2: 1e-12
    relative (the restatement on the host gives 2e-16)"""
    A, value = _field(name)
    ctx, post = _context(A, value)
    try:
        for normal, offset in PLANES[:3]:
            post = ctx.postprocess3d()
            whole = R.area(*ctx.download_level1(post))
            parts = []
            for below in (False, True):
                post = ctx.postprocess3d()
                out = ctx.level1_clip_plane(normal, offset, _flags(below))
                parts.append(R.area(*ctx.download_level1(out)))
            rel = abs(parts[0] + parts[1] - whole) / whole
            print(name, normal, offset, "areas", parts, "of", whole, "relative difference", rel)
            assert rel <= 1e-12
    finally:
        ctx.close()


# ---- 5. normals --------------------------------------------------------------------------------------------------------------
def _angle(a, b):
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.sum(a * b, axis=1))


def test_normals(tmp_path):
    from contourist_amd import tetrahedral, mesh_io
    A, value = _field("sphere")
    ctx, post = _context(A, value)
    worst = 0.0
    try:
        for normal, offset in PLANES[:3]:
            for below in (False, True):
                post = ctx.postprocess3d()
                pts, tris = ctx.download_level1(post)
                N = ctx.level1_normals(post)
                ref = R.clip(pts, tris, R.plane_scalars(pts, normal), offset, keep_below=below, normals=N)
                out = ctx.level1_clip_plane(normal, offset, _flags(below, normals=True))
                G = _after(ctx, out)
                _compare(out, ref, G, "normals %s %s" % (normal, below))
                N2 = ctx.level1_normals(out)
                ulps = np.abs(N2 - ref["normals"]) / np.spacing(np.maximum(np.abs(ref["normals"]), 2.0 ** -60))
                worst = max(worst, float(ulps.max()))
                assert N2.tobytes() == ref["normals"].tobytes()                                 # (the normalisation rounds as numpy's)
                old = G["lo_hi"][:, 0] == G["lo_hi"][:, 1]
                assert N2[old].tobytes() == N[G["lo_hi"][old, 0]].tobytes()                      # an old vertex keeps its normal
                # a cut vertex's normal lies within the angle its two end normals span (1e-12: the rounding of the angles themselves)
                a, b, n = N[G["lo_hi"][~old, 0]], N[G["lo_hi"][~old, 1]], N2[~old]
                span = _angle(a, b)
                assert np.all(_angle(a, n) <= span + 1e-12) and np.all(_angle(b, n) <= span + 1e-12)
                assert np.abs(np.linalg.norm(N2, axis=1) - 1.0).max() < 1e-15
        print("carried normals: largest difference to the restatement, in ulps:", worst)
        # a second clip carries the carried normals on
        pts, tris = ctx.download_level1(out)
        N = ctx.level1_normals(out)
        ref = R.clip(pts, tris, R.plane_scalars(pts, (0.0, 1.0, 0.0)), 22.6, normals=N)
        out2 = ctx.level1_clip_plane((0.0, 1.0, 0.0), 22.6, _flags(normals=True))
        _compare(out2, ref, _after(ctx, out2), "second clip")
        assert ctx.level1_normals(out2).tobytes() == ref["normals"].tobytes()
        # without the flag the normals calls answer UNSUPPORTED afterwards, and a clip that asks for them says so and changes nothing
        out3 = ctx.level1_clip_plane((0.0, 0.0, 1.0), 24.0, _flags())
        before = [x.tobytes() for x in ctx.download_level1(out3)]
        with pytest.raises(NotImplementedError):
            ctx.level1_normals(out3)
        with pytest.raises(NotImplementedError):
            ctx.level1_clip_plane((1.0, 0.0, 0.0), 30.0, _flags(normals=True))
        assert [x.tobytes() for x in ctx.download_level1(out3)] == before
    finally:
        ctx.close()
    # write_mesh(..., "ply_normals") of a clipped mesh reads back
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, value)
    counts = m.clip(plane=OBLIQUE)
    path = str(tmp_path / "clipped.ply")
    m.write_mesh(path, "ply_normals")
    P, T, Nf = mesh_io.read_ply(path, normals=True)
    ctx = m.context()
    pd, td = ctx.download_level1(m._post)
    assert len(P) == counts["n_vertices"] and P.tobytes() == pd.tobytes() and T.tobytes() == td.tobytes()
    assert Nf.tobytes() == m.vertex_normals().tobytes()


# ---- 6. sources --------------------------------------------------------------------------------------------------------------
def _mesh_bytes(ctx, out):
    p, t = ctx.download_level1(out)
    lo_hi, tt = ctx.level1_clip_map()
    return (p.tobytes(), t.tobytes(), ctx.download_level1_keys(out).tobytes(), lo_hi.tobytes(), tt.tobytes())


def test_sources():
    import torch
    from contourist_amd import tetrahedral
    A, value = _field("two_blobs")
    B = _ball(A.shape, (24.0, 20.0, 20.0), 14.5).astype(np.float32)                      # a second volume
    corner = tuple(n - 1 for n in A.shape)
    m = tetrahedral.GridContour3d(corner, A, value)
    m.get_points_and_triangles()
    ctx = m.context()

    def fresh():
        m._post = None
        m._ensure_post(True)
        return ctx.download_level1(m._post)
    pts, tris = fresh()
    s = m.vertex_values(B)
    ref = R.clip(pts, tris, s, -1.5)
    c1 = m.clip(scalars=s, value=-1.5, clean=False, normals=False)
    b1 = _mesh_bytes(ctx, m._post)
    assert c1["n_triangles"] == len(ref["triangles"]) > 0 and c1["n_cut_vertices"] == ref["n_cut_vertices"] > 0
    assert b1[0] == ref["points"].tobytes()
    fresh()
    c2 = m.clip(scalars=torch.from_numpy(s).to("cuda"), value=-1.5, clean=False, normals=False)
    assert c2 == c1 and _mesh_bytes(ctx, m._post) == b1                                    # numpy array and device tensor: the same bytes
    fresh()
    c3 = m.clip(field=B, value=-1.5, clean=False, normals=False)
    assert c3 == c1 and _mesh_bytes(ctx, m._post) == b1                                    # field=B is scalars=vertex_values(B)
    with pytest.raises(NotImplementedError):                                               # not on a derived mesh
        m.clip(field=B, value=-1.5)
    # clip_values carries an attribute of the caller's across the cut
    carried = m.clip_values(s)
    lo_hi, t = m.clip_map()
    assert np.array_equal(carried, R.carry(s, lo_hi, t)) and np.array_equal(lo_hi, ref["map_lo_hi"])
    assert carried.min() >= -1.5 - 1e-12
    cd = m.clip_values(torch.from_numpy(s).to("cuda"))
    assert cd.is_cuda and np.allclose(cd.cpu().numpy(), carried, rtol=0, atol=1e-15)
    ld, td = m.clip_map(device=True)
    assert np.array_equal(ld.cpu().numpy(), lo_hi) and np.array_equal(td.cpu().numpy(), t)
    # box= equals its six plane clips
    lo3, hi3 = (8.5, 12.0, 13.25), (30.0, 27.5, 26.0)
    fresh()
    cb = m.clip(box=(lo3, hi3), clean=False, normals=False)
    bb = _mesh_bytes(ctx, m._post)
    fresh()
    total = dict(n_cut_vertices=0, n_cut_triangles=0, n_nonfinite=0, n_on_cut=0)
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        for n, off in ((e, lo3[a]), (-e, -hi3[a])):
            cs = m.clip(plane=(n, off), clean=False, normals=False)
            for k in total:
                total[k] += cs[k]
    assert _mesh_bytes(ctx, m._post) == bb and cb["n_triangles"] == cs["n_triangles"] > 0
    assert {k: cb[k] for k in total} == total
    P = ctx.download_level1(m._post)[0]
    assert np.all(P >= np.array(lo3) - 1e-12) and np.all(P <= np.array(hi3) + 1e-12)
    # a box that misses the mesh stops early with an empty mesh
    fresh()
    ce = m.clip(box=((100.0, 0.0, 0.0), (101.0, 1.0, 1.0)))
    assert ce["n_triangles"] == 0 and ce["n_vertices"] == 0
    # NaN and inf scalars: their triangles are dropped and counted, nothing faults
    pts, tris = fresh()
    s2 = m.vertex_values(B)
    s2[::7] = np.nan
    s2[3::11] = np.inf
    s2[5::13] = -np.inf
    for below in (False, True):
        fresh()
        ref = R.clip(pts, tris, s2, -1.5, keep_below=below)
        out = ctx.level1_clip_scalars(s2, -1.5, _flags(below))
        assert ref["n_nonfinite"] > 0
        _compare(out, ref, _after(ctx, out), "non-finite scalars below=%s" % below)
    fresh()
    out = ctx.level1_clip_scalars(np.full(len(pts), np.nan), 0.0, _flags())
    assert out["n_triangles"] == 0 and out["n_nonfinite"] == len(tris)
    with pytest.raises(ValueError):
        fresh()
        ctx.level1_clip_scalars(np.zeros(3), 0.0)


# ---- 7. routes and state -----------------------------------------------------------------------------------------------------
def test_routes_and_state(tmp_path):
    from contourist_amd import _ffi, tetrahedral
    A, value = _field("two_blobs")
    corner = tuple(n - 1 for n in A.shape)
    fresh = _ffi.Context()
    fresh.upload_grid_native(A)
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    with pytest.raises(_ffi.CxError) as e:                                            # no post-pass
        fresh.level1_clip_plane((1.0, 0.0, 0.0), 20.5)
    assert e.value.code == _ffi.CX_ERR_INVALID
    with pytest.raises(_ffi.CxError) as e:
        fresh.level1_clip_map()
    assert e.value.code == _ffi.CX_ERR_STATE
    fresh.set_reference_corner(corner)
    fresh.shard_begin(0, A.shape[0] - 1)
    fresh.shard_finish([], [])
    with pytest.raises(NotImplementedError):                                          # a shard
        fresh.level1_clip_plane((1.0, 0.0, 0.0), 20.5)
    fresh.set_reference_corner((0, 0, 0))
    fresh.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    post = fresh.postprocess3d()
    before = [a.tobytes() for a in fresh.download_level1(post)]
    for bad in ((0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0)):             # a zero or non-finite normal
        with pytest.raises(_ffi.CxError) as e:
            fresh.level1_clip_plane(bad, 20.0)
        assert e.value.code == _ffi.CX_ERR_INVALID
    with pytest.raises(_ffi.CxError) as e:
        fresh.level1_clip_plane((1.0, 0.0, 0.0), 20.5, 8)                             # an unknown flag
    assert e.value.code == _ffi.CX_ERR_INVALID
    assert [a.tobytes() for a in fresh.download_level1(post)] == before
    with pytest.raises(_ffi.CxError) as e:
        fresh.level1_clip_map()
    assert e.value.code == _ffi.CX_ERR_STATE
    live0, allocs0 = _ffi.device_bytes(fresh.handle)
    out = fresh.level1_clip_plane((1.0, 0.0, 0.0), 20.5, _ffi.CX_CLIP_NORMALS)
    info = fresh.level1_clip_info()
    print("clip info", info, "device bytes before / after the first clip", live0, _ffi.device_bytes(fresh.handle)[0])
    # the edge table is sized by the cut corners, not by the mesh
    assert info["n_triangles_before"] == post["n_triangles"] and 0 < info["cut_corners"] <= 2 * out["n_cut_triangles"]
    assert info["table_slots"] < 4 * info["cut_corners"] + 2048 and info["table_slots"] < 3 * post["n_triangles"]
    assert _ffi.device_bytes(fresh.handle)[0] > live0
    # a second clip of the same mesh allocates nothing
    fresh.postprocess3d()
    fresh.level1_clip_plane((1.0, 0.0, 0.0), 20.5, _ffi.CX_CLIP_NORMALS)
    live1, allocs1 = _ffi.device_bytes(fresh.handle)
    fresh.postprocess3d()
    fresh.level1_clip_plane((1.0, 0.0, 0.0), 20.5, _ffi.CX_CLIP_NORMALS)
    assert _ffi.device_bytes(fresh.handle) == (live1, allocs1)
    fresh.close()
    # a slab-marched (cx_postprocess3d_mesh) source: no normals there; normals="auto" works without them
    m = tetrahedral.GridContour3d(corner, A, value)
    m.MAX_SAMPLES_PER_EXTRACTION = 40 * 40 * 12
    assert m._in_slabs()
    ctx = m._ensure_post(True)
    before = [a.tobytes() for a in ctx.download_level1(m._post)]
    with pytest.raises(NotImplementedError):
        ctx.level1_clip_plane((1.0, 0.0, 0.0), 20.5, _ffi.CX_CLIP_NORMALS)
    assert [a.tobytes() for a in ctx.download_level1(m._post)] == before
    pts, tris = ctx.download_level1(m._post)
    ref = R.clip(pts, tris, R.plane_scalars(pts, (1.0, 0.0, 0.0)), 20.5)
    cs = m.clip(plane=((1.0, 0.0, 0.0), 20.5), clean=False)
    assert cs["n_triangles"] == len(ref["triangles"]) > 0 and ctx.download_level1(m._post)[0].tobytes() == ref["points"].tobytes()
    with pytest.raises(NotImplementedError):
        m.vertex_normals()
    # the Python layer after a clip
    m = tetrahedral.GridContour3d(corner, A, value)
    full = m.get_points_and_triangles()
    with pytest.raises(ValueError):
        m.clip()
    with pytest.raises(ValueError):
        m.clip(plane=((0.0, 0.0, 0.0), 1.0))
    with pytest.raises(_ffi.CxError) as e:
        m.clip_map()
    assert e.value.code == _ffi.CX_ERR_STATE
    cs = m.clip(plane=((1.0, 0.0, 0.0), 20.5))
    assert set(cs) == set(_ffi.CLIP_KEYS) and 0 < cs["n_triangles"] and cs["n_components"] == 2 and cs["n_cut_vertices"] > 0
    with pytest.raises(NotImplementedError):
        m.vertex_values(A)
    with pytest.raises(NotImplementedError):
        m.vertex_curvature()
    P, T = m.get_points_and_triangles()
    assert len(P) == cs["n_vertices"] and len(T) == cs["n_triangles"] and P[:, 0].min() >= 20.5 - 1e-12
    N = m.vertex_normals()
    assert N.shape == P.shape and np.abs(np.linalg.norm(N, axis=1) - 1.0).max() < 1e-12
    assert len(m.components()) == 2 and len(m.clip_map()[1]) == len(P)
    with pytest.raises(_ffi.CxError) as e:
        m.simplify_map()
    assert e.value.code == _ffi.CX_ERR_STATE
    m.write_mesh(str(tmp_path / "half.ply"), "ply")
    kept = m.keep_components(largest=1)
    assert kept["n_components"] == 1 and m.vertex_normals().shape == (kept["n_vertices"], 3)
    with pytest.raises(_ffi.CxError) as e:                                            # the filter ends the map's life
        m.clip_map()
    assert e.value.code == _ffi.CX_ERR_STATE
    c2 = m.clip(plane=((0.0, 1.0, 0.0), 20.0), keep="below")                          # a second clip
    assert 0 < c2["n_triangles"] and len(m.clip_map()[1]) == c2["n_vertices"]
    sm = m.simplify(cell=2.0)
    assert 0 < sm["n_triangles"] < c2["n_triangles"] and len(m.simplify_map()) == c2["n_vertices"]
    assert m.vertex_normals().shape == (sm["n_vertices"], 3)
    with pytest.raises(_ffi.CxError) as e:                                            # after a later simplify()
        m.clip_map()
    assert e.value.code == _ffi.CX_ERR_STATE
    m.march(force=True)                                                               # a new march resets everything
    again = m.get_points_and_triangles()
    assert np.array_equal(again[0], full[0]) and np.array_equal(again[1], full[1])
    assert m.vertex_values(A).shape == (len(full[0]),) and m.vertex_curvature().shape == (len(full[0]), 4)


def test_levels_and_world_coordinates():
    "LevelResult.clip and Delta3DContour.clip: the plane in world coordinates"
    from contourist_amd import tetrahedral, _ffi
    A, value = _field("two_blobs")
    mins, delta = np.array([0.5, 1.0, -2.0]), np.array([0.5, 1.0, 2.0])
    n_w, off_w = np.array([0.6, -0.3, 0.2]), 0.6 * 12.0 - 0.3 * 20.0 + 0.2 * 38.0
    n_g, off_g = n_w * delta, off_w - float(np.dot(n_w, mins))
    M = tetrahedral.MultiLevelIsosurfaces(mins, None, delta, A, [-1.0, 0.5])
    seen = 0
    for lv in M.levels():
        ctx = lv._ctx()
        pts, tris = ctx.download_level1(lv._post)
        ref = R.clip(pts, tris, R.plane_scalars(pts, n_g), off_g)
        counts = lv.clip(plane=(n_w, off_w), clean=False)
        assert set(counts) == set(_ffi.CLIP_KEYS) and counts["n_triangles"] == len(ref["triangles"]) > 0
        P, T = lv.mesh()
        assert np.array_equal(P, ref["points"] * delta + mins) and len(T) == len(ref["triangles"])
        assert np.all(P @ n_w >= off_w - 1e-9)
        assert np.array_equal(lv.clip_map()[0], ref["map_lo_hi"]) and lv.vertex_normals().shape == P.shape
        assert np.array_equal(lv.clip_values(pts[:, 0]), R.carry(pts[:, 0], ref["map_lo_hi"], ref["map_t"]))
        with pytest.raises(NotImplementedError):
            lv.vertex_values(A)
        seen += 1
    assert seen == 2
    S = tetrahedral.TriangulatedIsosurfaces(list(mins), None, list(delta), A, value, [])
    S.search_for_endpoints()
    maker = S.contour_maker
    S.get_points_and_triangles()
    ctx = maker.context()
    pts, tris = ctx.download_level1(maker._post)
    ref = R.clip(pts, tris, R.plane_scalars(pts, n_g), off_g, keep_below=True)
    counts = S.clip(plane=(n_w, off_w), keep="below", clean=False)
    assert counts["n_triangles"] == len(ref["triangles"]) > 0
    P, T = S.get_points_and_triangles()
    assert np.array_equal(P, S.grid.from_grid_coordinates(ref["points"])) and np.all(P @ n_w <= off_w + 1e-9)
    assert np.array_equal(S.clip_map()[0], ref["map_lo_hi"])


# ---- 8. reproducibility ------------------------------------------------------------------------------------------------------
def test_bit_identical():
    A, value = _field("noise")
    blobs = []
    for k in range(2):
        ctx, post = _context(A, value)
        for again in range(2 if k == 0 else 1):
            post = ctx.postprocess3d()
            out = ctx.level1_clip_plane(OBLIQUE[0], OBLIQUE[1] + 20.0, _flags(clean=True, normals=True))
            blobs.append(_mesh_bytes(ctx, out) + (ctx.level1_normals(out).tobytes(), repr(sorted(out.items()))))
        ctx.close()
    assert len(blobs) == 3 and blobs[0][0] and all(b == blobs[0] for b in blobs[1:])
