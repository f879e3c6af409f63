"""Rim caps on the device (cx_cap.hip) against tests/cap_ref.py, the numpy restatement of the header's section "rim caps".

Raw parity: keys, triangles and counts of cx_cap3d_download, bit for bit, with the restatement run on the DEVICE's Level-0 keys (the
cap names Level-0 vertices by their index).  Level-1 parity: cx_postprocess3d_capped against oracle.postpass.level1_from_level0 on
(the oracle's Level 0 + the restatement's cap) through oracle.postpass.compare_level1.  The fields are cap_ref.field(): the constant
5x4x3 one (rows shorter than 4 samples: the shape-agnostic march), the plane, the cut sphere (off the lattice for the closedness
assertions, and as the issue wrote it, with a rim sample EQUAL to the isovalue, for parity only), white noise 14x20x26, smoothed noise
33x17x66 (a row spans more than one 64-lane word) and a uint8 grid."""
import numpy as np
import pytest

import cap_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
_shared = {}


@pytest.fixture(scope="module")
def extraction():
    "one context per field, marched once: (context, samples, value, Level-0 counts, the device's Level-0 keys and triangles)"
    from contourist_amd import _ffi

    def get(name):
        if name not in _shared:
            A, v = R.field(name)
            ctx = _ffi.Context()
            ctx.upload_grid_native(A)
            c = ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
            keys0, _t, tris0 = ctx.download_level0_records(c)
            _shared[name] = (ctx, A, v, c, keys0, tris0)
        return _shared[name]
    yield get
    for entry in _shared.values():
        entry[0].close()
    _shared.clear()


_oracle = {}


def _straddling_pair(A, v):
    "two neighbouring lattice points along k on either side of the isovalue, from the middle of the array: end points of a seeded selection"
    low = np.asarray(A).astype(np.float64) < v
    hits = np.argwhere(low[:, :, :-1] != low[:, :, 1:])
    i, j, k = (int(x) for x in hits[len(hits) // 2])
    return [((i, j, k), (i, j, k + 1))]


def _oracle_level1(name, mask, side):
    "Level 1 of (the oracle's Level 0 + the restatement's cap), once per case"
    key = (name, mask, side)
    if key not in _oracle:
        from oracle import level0, postpass
        A, v = R.field(name)
        O = level0.march3d(A.astype(np.float32), v, diag_mode=1)
        keys0 = level0.edge_keys_from_pairs(O["pairs"], A.shape)
        keys, xyz, tris, C = R.capped_level0(A, v, mask, side, keys0, O["xyz"], O["tris"])
        _oracle[key] = (postpass.level1_from_level0(keys, xyz, tris, np.array(A.shape) - 1), C)
    return _oracle[key]


# ---- 1. the raw cap, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FIELDS)
def test_raw_parity(name, extraction):
    ctx, A, v, c, keys0, tris0 = extraction(name)
    if name == "constant":
        assert c["n_triangles"] == 0 and A.shape[2] < 4
    if name == "sphere_exact":
        assert A[0, 4, 4] == v                                   # a rim sample equal to the isovalue
    assert len(np.unique(keys0)) == len(keys0)
    for side in ("above", "below"):
        for mask in R.MASKS:
            what = (name, side, hex(mask))
            counts = ctx.cap3d(mask, side)
            keys, tris = ctx.download_cap(counts)
            ref = R.cap(A, v, mask, side, keys0)
            assert [counts[k] for k in R.COUNT_KEYS] == ref["counts"].tolist(), what
            assert keys.tobytes() == ref["keys"].tobytes(), what
            assert tris.dtype == np.int32 and tris.tobytes() == ref["triangles"].tobytes(), what
            assert ctx.cap3d(mask, side) == counts                                     # idempotent
            k2, t2 = ctx.download_cap(counts)
            assert k2.tobytes() == keys.tobytes() and t2.tobytes() == tris.tobytes(), what
            # the raw concatenation with the DEVICE's march: every shared edge runs in opposite directions, before any orientation step
            both = np.concatenate([tris0.astype(np.int64).reshape(-1, 3), tris.astype(np.int64).reshape(-1, 3)])
            boundary, nonmanifold, incoherent, _euler = R.edge_uses(both)
            if name != "sphere_exact":
                assert counts["n_missing_crossings"] == 0 and (nonmanifold, incoherent) == (0, 0), (what, nonmanifold, incoherent)
                if mask == 0x3F:
                    assert boundary == 0, what
            if mask == 0:
                assert len(keys) == 0 and len(tris) == 0 and counts["n_rim_crossings"] == 0


# ---- 2. Level 1 of march + cap ----------------------------------------------------------------------------------------------------
_L1_CASES = [("constant", "below"), ("constant", "above"), ("plane", "above"), ("plane", "below"), ("sphere", "above"), ("sphere", "below"),
             ("sphere_exact", "above"), ("sphere_exact", "below"), ("noise_14x20x26", "above"), ("noise_33x17x66", "above"), ("noise_u8", "below")]


@pytest.mark.parametrize("name,side", _L1_CASES)
def test_level1_parity(name, side, extraction):
    from oracle import postpass
    ctx, A, v, c, keys0, tris0 = extraction(name)
    corner = np.array(A.shape) - 1
    L1, C = _oracle_level1(name, 0x3F, side)
    counts = ctx.cap3d(0x3F, side)
    assert [counts[k] for k in R.COUNT_KEYS] == C["counts"].tolist()
    for clean in (True, False):
        post = ctx.postprocess3d_capped(0 if clean else 1)
        assert post["n_after_weld"] == L1["n_after_weld"] and post["n_after_tiny"] == L1["n_after_tiny"], (name, side, clean, post)
        pts, tris = ctx.download_level1(post)
        assert tris.min(initial=0) >= 0 and tris.max(initial=-1) < len(pts)
        if not clean:
            assert post["n_triangles"] == L1["n_after_tiny"]
            continue
        assert len(tris) == len(L1["triangles"]), (name, side)
        cmp = postpass.compare_level1(L1, pts, tris, corner, reach=0 if name != "sphere_exact" else 2)
        assert not cmp["missing"] and not cmp["extra"] and not cmp["winding"], (name, side, {k: (len(x) if isinstance(x, list) else x) for k, x in cmp.items()})
        if name != "sphere_exact":
            assert cmp["excused_rows"] == 0
            assert R.edge_uses(tris)[:3] == (0, 0, 0), (name, side)
        # the keys that come back: edge ids and lattice points, the points by the post-pass's formula, bit for bit
        keys = ctx.download_level1_keys(post)
        assert pts.tobytes() == R.points(A, v, keys).tobytes(), (name, side)
        if len(keys):
            assert np.count_nonzero(keys & 7 == 0) > 0


# ---- 3. what the device says about the closed mesh -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,side,volume,omit", [("plane", "above", 90.0, "+x"), ("plane", "below", 50.0, "-x"), ("sphere", "above", None, "-x"),
                                                   ("sphere", "below", None, "-x")])
def test_device_facts(name, side, volume, omit, extraction):
    "omit: a face the solid reaches (the solid i >= 2.5 of the plane field does not reach i = 0)"
    ctx, A, v, c, keys0, tris0 = extraction(name)
    ctx.postprocess3d()
    assert ctx.level1_topology()["boundary_edges"].sum() > 0 and not ctx.level1_components()["closed"].any()          # uncapped: open
    assert len(ctx.level1_boundary_loops()[0]) > 0
    ctx.cap3d("all", side)
    post = ctx.postprocess3d_capped()
    topo = ctx.level1_topology()
    assert len(topo) == 1 and topo["boundary_edges"][0] == 0 and topo["nonmanifold_edges"][0] == 0 and topo["euler"][0] == 2 and topo["genus"][0] == 0
    table, origin, q = ctx.level1_components(info=True)
    assert len(table) == 1 and table["closed"][0] == 1
    loops, verts = ctx.level1_boundary_loops()
    assert len(loops) == 0 and len(verts) == 0
    pts, tris = ctx.download_level1(post)
    if volume is None:
        volume = abs(R.signed_volume(pts - origin, tris))
        print(name, side, "volume", float(table["volume"][0]), "float64 sum", volume)
    # the tolerance tests/test_gpu_components.py holds a closed mesh's volume to: the grid 2^-q of the sums and 16 ulp of the sum of the
    # terms' magnitudes (the plane field's points are exact, so 90 and 50 are the exact volumes of the mesh)
    a, b, cc = (pts[tris[:, k]] - origin for k in range(3))
    P_vol = (np.abs(a[:, 0] * b[:, 1] * cc[:, 2]) + np.abs(a[:, 0] * b[:, 2] * cc[:, 1]) + np.abs(a[:, 1] * b[:, 2] * cc[:, 0]) +
             np.abs(a[:, 1] * b[:, 0] * cc[:, 2]) + np.abs(a[:, 2] * b[:, 0] * cc[:, 1]) + np.abs(a[:, 2] * b[:, 1] * cc[:, 0])).sum() / 6.0
    bound = len(tris) * 2.0 ** -(q + 1) + 16 * EPS * P_vol
    print(name, side, "volume", float(table["volume"][0]), "bound", bound)
    assert abs(table["volume"][0] - volume) <= bound, (table["volume"][0], volume, bound)
    # one face left open: the loops that remain lie in it
    ctx.cap3d([f for f in R.FACE_NAMES if f != omit], side)
    post = ctx.postprocess3d_capped()
    pts, tris = ctx.download_level1(post)
    loops, verts = ctx.level1_boundary_loops()
    assert len(loops) > 0 and np.all(pts[verts][:, 0] == (0.0 if omit == "-x" else A.shape[0] - 1.0))
    assert not ctx.level1_components()["closed"].all()


# ---- 4. nothing changes without a request; lifetime; refusals -----------------------------------------------------------------------
def test_plain_postpass_is_unchanged_by_a_cap_round_trip():
    from contourist_amd import tetrahedral
    A, v = R.field("sphere")
    maker = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, v)
    try:
        ctx = maker._ensure_post()
        before = (ctx.download_level1(maker._post), ctx.download_level1_keys(maker._post))
        counts = maker.cap_rim()
        assert counts["n_cap_triangles"] > 0 and maker._post is None
        pc, tc = maker.get_points_and_triangles()
        assert R.edge_uses(tc)[:2] == (0, 0) and len(tc) > len(before[0][1])
        assert maker.cap_rim(None) is None
        ctx = maker._ensure_post()
        after = (ctx.download_level1(maker._post), ctx.download_level1_keys(maker._post))
        assert before[0][0].tobytes() == after[0][0].tobytes() and before[0][1].tobytes() == after[0][1].tobytes() and before[1].tobytes() == after[1].tobytes()
        assert "capped" not in maker._post
    finally:
        maker.context().close()


def test_lifetime(extraction):
    from contourist_amd import _ffi
    A, v = R.field("noise_14x20x26")
    ctx = _ffi.Context()
    try:
        ctx.upload_grid_native(A)
        with pytest.raises(_ffi.CxError) as e:
            ctx.cap3d("all", "above")
        assert e.value.code == _ffi.CX_ERR_STATE
        c = ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        with pytest.raises(_ffi.CxError) as e:
            ctx.postprocess3d_capped()
        assert e.value.code == _ffi.CX_ERR_STATE                      # no cap yet
        counts = ctx.cap3d("all", "above")

        def gone():
            for call in (lambda: ctx.download_cap(counts), ctx.postprocess3d_capped):
                with pytest.raises(_ffi.CxError) as e:
                    call()
                assert e.value.code == _ffi.CX_ERR_STATE
        ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)                    # a new extraction, even of the same value
        gone()
        ctx.cap3d("all", "above")
        ctx.extract3d_levels([-0.2, 0.3], _ffi.CX_DIAG_CPYTHON310)
        gone()
        ctx.select_level(0)
        c0 = ctx.cap3d("all", "above")
        ctx.select_level(1)
        gone()
        ctx.select_level(0)
        gone()
        assert ctx.cap3d("all", "above") == c0
        ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        ctx.cap3d("all", "above")
        ctx.select_seeded(_straddling_pair(A, v))
        gone()
        ctx.upload_grid_native(A)                                     # a grid call
        gone()
    finally:
        ctx.close()


def test_refusals():
    from contourist_amd import _ffi
    A, v = R.field("sphere")
    ctx = _ffi.Context()

    def refused(call, code=_ffi.CX_ERR_UNSUPPORTED):
        with pytest.raises(_ffi.CxError) as e:
            call()
        assert e.value.code == code, e.value
    try:
        ctx.upload_grid_native(A)
        c = ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        post = ctx.postprocess3d()
        before = (ctx.download_level1(post), ctx.download_level1_keys(post))

        def untouched():
            p, t = ctx.download_level1(post)
            assert p.tobytes() == before[0][0].tobytes() and t.tobytes() == before[0][1].tobytes() and ctx.download_level1_keys(post).tobytes() == before[1].tobytes()
        assert ctx.lib.cx_cap3d(ctx.handle, 64, 0, None) == _ffi.CX_ERR_INVALID and ctx.lib.cx_cap3d(ctx.handle, 63, 2, None) == _ffi.CX_ERR_INVALID
        # a seeded selection in force
        ctx.select_seeded(_straddling_pair(A, v))
        refused(lambda: ctx.cap3d("all", "above"))
        ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        post = ctx.postprocess3d()
        untouched()
        # arrays carrying a margin: a negative origin, a reference corner; a slab: a positive origin
        for setup, undo in ((lambda: ctx.set_origin(-1, -1, -1), lambda: ctx.set_origin(0, 0, 0)),
                            (lambda: ctx.set_reference_corner((18, 18, 18)), lambda: ctx.set_reference_corner((0, 0, 0))),
                            (lambda: ctx.set_origin(20, 0, 0), lambda: ctx.set_origin(0, 0, 0))):
            ctx.cap3d("all", "above")                                 # a valid cap is no licence either
            setup()
            refused(lambda: ctx.cap3d("all", "below"))
            refused(ctx.postprocess3d_capped)
            undo()
            post = ctx.postprocess3d()
            untouched()
        # the caller's-mesh and shard routes take no cap: they leave a plain mesh, and the capped entry needs its own cap
        ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        refused(ctx.postprocess3d_capped, _ffi.CX_ERR_STATE)
    finally:
        ctx.close()
    from contourist_amd import tetrahedral
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, v)
    try:
        m.cap_rim()
        m.smooth = 0.5                                                # smoothing asked for after the cap
        with pytest.raises(NotImplementedError, match="smooth"):
            m.get_points_and_triangles()
    finally:
        m.context().close()


# ---- 5. attributes, levels, reproducibility, downstream ------------------------------------------------------------------------------
def test_normals_are_refused_and_values_sample_the_lattice(tmp_path):
    from contourist_amd import tetrahedral
    A, v = R.field("sphere")
    rng = np.random.default_rng(3)
    B = rng.normal(size=A.shape).astype(np.float32)
    m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, v)
    try:
        plain = m.vertex_normals()
        assert plain.shape[1] == 3
        m.cap_rim("all", "above")
        for call in (m.vertex_normals, m.vertex_curvature, lambda: m.write_mesh(str(tmp_path / "n.ply"), "ply_normals")):
            with pytest.raises(NotImplementedError, match="capped"):
                call()
        info = m.write_mesh(str(tmp_path / "c.ply"), "ply")
        pts, tris = m.get_points_and_triangles()
        assert info["n_triangles"] == len(tris)
        ctx = m.context()
        keys = ctx.download_level1_keys(m._post)
        vals = ctx.level1_sample(m._post, B)
        lat = keys & 7 == 0
        assert lat.any() and vals[lat].tobytes() == B.reshape(-1)[keys[lat] >> 3].astype(np.float64).tobytes()
        own = ctx.level1_sample(m._post, A)                          # the field itself: the isovalue at the crossings, f at the lattice points
        assert np.abs(own[~lat] - v).max() < 1e-5 and np.all(own[lat] >= v)
        # a filtered copy of a capped mesh is still a capped mesh
        m.keep_components(largest=1)
        with pytest.raises(NotImplementedError, match="capped"):
            m.vertex_normals()
        m.cap_rim(None)
        assert m.vertex_normals().tobytes() == plain.tobytes()
    finally:
        m.context().close()


def test_levels_with_a_cap_equal_single_capped_calls():
    from contourist_amd import tetrahedral
    A, _v = R.field("noise_33x17x66")
    values = [-0.03, 0.02]                 # both inside the band the field keeps clear of samples: the closedness below needs it
    assert all(np.abs(A.astype(np.float64) - val).min() > 1e-3 for val in values)
    M = tetrahedral.MultiLevelIsosurfaces((0, 0, 0), tuple(n - 1 for n in A.shape), (1, 1, 1), A, values)
    got = [(val, np.array(p), np.array(t), r.topology()) for r in M.levels(cap="all") for (val, p, t) in [tuple(r)]]
    assert [g[0] for g in got] == values
    for val, p, t, topo in got:
        S = tetrahedral.TriangulatedIsosurfaces((0, 0, 0), tuple(n - 1 for n in A.shape), (1, 1, 1), A, val, None)
        S.cap_rim("all")
        ps, ts = S.get_points_and_triangles()
        assert np.asarray(ps).tobytes() == p.tobytes() and np.asarray(ts).tobytes() == t.tobytes(), val
        assert topo["boundary_edges"].sum() == 0 and np.array_equal(topo, S.topology())
        S.contour_maker.context().close()
    plain = [np.array(t) for (_val, _p, t) in M.levels()]
    assert all(len(a) < len(g[2]) for a, g in zip(plain, got))


def test_two_calls_give_the_same_bytes():
    from contourist_amd import _ffi
    A, v = R.field("noise_33x17x66")
    out = []
    for _ in range(2):
        ctx = _ffi.Context()
        ctx.upload_grid_native(A)
        ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
        for rep in range(2):
            counts = ctx.cap3d("all", "below")
            post = ctx.postprocess3d_capped()
            out.append((ctx.download_cap(counts), ctx.download_level1(post), ctx.download_level1_keys(post)))
        ctx.close()
    for o in out[1:]:
        assert o[0][0].tobytes() == out[0][0][0].tobytes() and o[0][1].tobytes() == out[0][0][1].tobytes()
        assert o[1][0].tobytes() == out[0][1][0].tobytes() and o[1][1].tobytes() == out[0][1][1].tobytes() and o[2].tobytes() == out[0][2].tobytes()


def test_downstream_simplify_and_clip():
    from contourist_amd import tetrahedral
    A, v = R.field("sphere")
    for step in ("simplify", "clip"):
        m = tetrahedral.GridContour3d(tuple(n - 1 for n in A.shape), A, v)
        try:
            m.cap_rim()
            closed = m.topology()
            assert closed["boundary_edges"].sum() == 0
            if step == "simplify":
                m.simplify(cell=2, normals=False)
            else:
                m.clip(plane=((0.0, 1.0, 0.0), 10.4), normals=False)
            pts, tris = m.get_points_and_triangles()
            pts, tris = np.asarray(pts), np.asarray(tris)
            assert len(tris) > 0 and tris.min() >= 0 and tris.max() < len(pts)
            if step == "clip":
                assert np.all(pts[:, 1] >= 10.4 - 1e-12) and m.topology()["boundary_edges"].sum() > 0
        finally:
            m.context().close()
