"""GPU: a 4-D volume of more than GridContour4D.MAX_SAMPLES_PER_EXTRACTION samples is marched slab by slab along axis 0 and assembled
on the device (cx_slab4d_begin / _append / _finish).  With the limit lowered, every result keyed by global edge id equals the single
extraction of the same array: find_tetrahedra's points bit for bit, its tetrahedra (the order of their four corners, i.e. their
orientation, included), the morph segments and triangles with their windings, the components and the surfaces at several times.
Beyond the real limit (2^28 samples) the assembly is checked through size-independent properties."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (40, 24, 20, 16)
PLANE = SHAPE[1] * SHAPE[2] * SHAPE[3]


def _smooth(shape, seed, passes=3):
    rng = np.random.RandomState(seed)
    A = rng.standard_normal(shape)
    for _ in range(passes):
        for axis in range(4):
            A = (np.roll(A, 1, axis) + 2.0 * A + np.roll(A, -1, axis)) / 4.0
    return (A - A.mean()) / A.std()


def smooth_noise(shape=SHAPE, seed=5):
    return np.ascontiguousarray(_smooth(shape, seed), dtype=np.float32), 0.0


def moving_blobs(shape=SHAPE, seed=6):
    ax = [np.linspace(0.0, 1.0, n) for n in shape]
    X, Y, Z, T = np.meshgrid(*ax, indexing="ij")
    A = np.exp(-(((X - 0.25 - 0.4 * T) ** 2 + (Y - 0.45) ** 2 + (Z - 0.5) ** 2) / (2 * 0.12 ** 2))) + \
        np.exp(-(((X - 0.75 + 0.35 * T) ** 2 + (Y - 0.55) ** 2 + (Z - 0.45 + 0.1 * T) ** 2) / (2 * 0.10 ** 2)))
    A = A + 0.02 * _smooth(shape, seed, 2)
    return np.ascontiguousarray(A, dtype=np.float32), 0.5


def quantised(shape=SHAPE, seed=7):
    "samples on a grid of quarters: many EQUAL the isovalue 0 (tetrahedra on lattice planes, vertices shared across slab planes)"
    A = np.round(4.0 * _smooth(shape, seed)) / 4.0
    assert np.mean(A == 0.0) > 0.05
    return np.ascontiguousarray(A, dtype=np.float32), 0.0


FIELDS = {"smooth_noise": smooth_noise, "moving_blobs": moving_blobs, "quantised": quantised}


def _limit(planes):
    "the limit that makes _slab_planes() == planes on SHAPE"
    return (planes + 1) * PLANE


def _canon_tets(keys, tets):
    "tetrahedra as rows of global edge ids in the order of their corners (the orientation), rows sorted"
    K = np.asarray(keys, dtype=np.int64)[np.asarray(tets, dtype=np.int64)]
    return K[np.lexsort(K.T[::-1])]


def _morph_arrays(m):
    "(points4d, segments, triangles) the context holds after collect_morph_triangles"
    pts, segs, tris, _ = m.context().morph_triangles()
    return pts, segs, tris


def _canon_segments(keys, segs):
    K = np.asarray(keys, dtype=np.int64)[np.asarray(segs, dtype=np.int64)]
    return K[np.lexsort(K.T[::-1])]


def _canon_triangles(keys, segs, tris, oriented=True):
    """triangles as key-pair triples: rotated (winding kept) so that the smallest pair comes first, or with oriented=False the three
    pairs sorted; rows sorted"""
    K = np.asarray(keys, dtype=np.int64)[np.asarray(segs, dtype=np.int64)]          # (S, 2) key pairs
    T = K[np.asarray(tris, dtype=np.int64)].reshape(-1, 3, 2)                         # (T, 3, 2)
    w = T[:, :, 0] * (1 << 40) + T[:, :, 1]
    rows = np.arange(len(T))
    if oriented:
        r = np.argmin(w, axis=1)
        T = np.stack([T[rows, r], T[rows, (r + 1) % 3], T[rows, (r + 2) % 3]], axis=1)
    else:
        T = T[rows[:, None], np.argsort(w, axis=1)]
    T = T.reshape(-1, 6)
    return T[np.lexsort(T.T[::-1])]


def _canon_surface(pts, tris, oriented=True):
    """a surface at time t as rows of 9 coordinates: corners rotated to start at the smallest (winding kept), or with oriented=False
    sorted; rows sorted.  And the sorted points (bits)"""
    P = np.asarray(pts, dtype=np.float64)
    C = P[np.asarray(tris, dtype=np.int64)]                            # (Q, 3, 3)
    rows = np.arange(len(C))
    rank = np.empty((len(C), 3), dtype=np.int64)                       # lexicographic rank of each corner inside its triangle
    for c in range(3):
        a = C[:, c]
        rank[:, c] = sum(((C[:, o, 0] < a[:, 0]) | ((C[:, o, 0] == a[:, 0]) & ((C[:, o, 1] < a[:, 1]) | ((C[:, o, 1] == a[:, 1]) & (C[:, o, 2] < a[:, 2])))))
                         .astype(np.int64) for o in range(3))
    if oriented:
        best = np.argmin(rank, axis=1)
        R = np.stack([C[rows, best], C[rows, (best + 1) % 3], C[rows, (best + 2) % 3]], axis=1)
    else:
        R = C[rows[:, None], np.argsort(rank * 3 + np.arange(3), axis=1)]
    R = R.reshape(-1, 9)
    return R[np.lexsort(R.T[::-1])], np.sort(P.view(np.int64).reshape(-1, 3), axis=0)


def _compare(ref, got, windings=True):
    """windings=False: the windings of a component whose start triangle (the orientation rule of surface_geometry.py:79-103 on the
    segment midpoints) is picked by a tie -- several segments at the component's largest x, several triangles with the same |normal x|
    -- follow the numbering of the segments, which differs between the two paths (and between two single extractions whose march
    numbers its vertices differently): the triangles are compared without winding, and every surface must be wound as consistently as
    the single extraction's (the same number of manifold edges run twice in one direction)"""
    from test_gpu_fullsize import edge_consistency
    # find_tetrahedra: points bit for bit by global edge id, counts, tetrahedra with their corner order
    k0 = np.asarray(ref["ft"]["keys"], dtype=np.int64)
    o = np.argsort(k0)
    k1 = got["ft"]["keys"]
    assert k1.dtype == np.int64 and np.all(np.diff(k1) > 0)                  # ascending global edge id
    assert np.array_equal(k0[o], k1)
    assert np.array_equal(ref["ft"]["points4d"][o].view(np.int64), got["ft"]["points4d"].view(np.int64))
    assert ref["ft"]["counts"] == got["ft"]["counts"]
    assert np.array_equal(_canon_tets(k0, ref["ft"]["tetrahedra"]), _canon_tets(k1, got["ft"]["tetrahedra"]))
    # morph triangles: segments as key pairs, triangles as key-pair triples up to rotation (windings included), components
    pr, sr, tr = ref["morph"]
    pg, sg, tg = got["morph"]
    assert len(sr) == len(sg) and len(tr) == len(tg)
    assert np.array_equal(_canon_segments(k0, sr), _canon_segments(k1, sg))
    assert np.array_equal(_canon_triangles(k0, sr, tr, windings), _canon_triangles(k1, sg, tg, windings))
    assert ref["ncomp"] == got["ncomp"]
    # the surfaces at 8 times
    for (p0, t0), (p1, t1) in zip(ref["surf"], got["surf"]):
        assert len(t0) == len(t1) and len(p0) == len(p1)
        a, b = _canon_surface(p0, t0, windings), _canon_surface(p1, t1, windings)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        if not windings:
            assert edge_consistency(t0) == edge_consistency(t1)


def _with_morph(A, value, limit, on_device, times):
    import torch
    from contourist_amd import pentatopes
    S = torch.from_numpy(A).cuda() if on_device else A
    m = pentatopes.GridContour4D(tuple(n - 1 for n in A.shape), S, value)
    if limit is not None:
        m.MAX_SAMPLES_PER_EXTRACTION = limit
        assert m._in_slabs()
    else:
        assert not m._in_slabs()
    ft = m.find_tetrahedra()
    m.collect_morph_triangles()
    morph = _morph_arrays(m)
    ncomp = m.n_components
    if times is None:
        t = morph[0][:, 3]
        times = list(np.linspace(float(t.min()), float(t.max()), 10)[1:-1])
    surf = m.triangles_at_many(times)
    out = dict(ft=ft, morph=morph, ncomp=ncomp, surf=[(np.array(p), np.array(q)) for p, q in surf], times=times,
               slab_counts=getattr(m, "_slab_counts", None))
    m.context().close()
    return out


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_slabs_equal_the_single_extraction(field):
    """2, 3 and 5 slabs, a last slab that absorbs a trailing plane, host array and device tensor: everything keyed by global edge id
    equals the single extraction of the same array"""
    pytest.importorskip("torch")
    A, value = FIELDS[field]()
    ref = _with_morph(A, value, None, False, None)
    assert len(ref["ft"]["tetrahedra"]) > 1000 and len(ref["morph"][2]) > 1000
    for planes, on_device, n_slabs in ((20, False, 2), (14, True, 3), (8, False, 5), (13, True, 3)):
        got = _with_morph(A, value, _limit(planes), on_device, ref["times"])
        assert got["slab_counts"]["n_slabs"] == n_slabs
        _compare(ref, got, windings=(field == "moving_blobs"))      # (two closed blobs: no tie decides a component's winding)


def test_the_trailing_plane_joins_the_last_slab():
    from contourist_amd import pentatopes
    assert pentatopes.GridContour4D._slab_bounds(SHAPE[0], 13) == [(0, 13), (13, 26), (26, 40)]


def test_many_thin_slabs_regrow_the_assembly():
    """slabs of two planes (the last of three): ~20 appends, so that every assembly buffer grows several times; the result is the
    single extraction's"""
    pytest.importorskip("torch")
    A, value = quantised((41, 24, 20, 16), 11)
    ref = _with_morph(A, value, None, False, None)
    got = _with_morph(A, value, 3 * PLANE, True, ref["times"])
    assert got["slab_counts"]["n_slabs"] == 20
    _compare(ref, got, windings=False)


def test_assembly_abi_order_and_state():
    """the C ABI refuses a slab out of order, a post-pass between begin and finish, a finish with planes missing; a later
    extraction invalidates the assembled result"""
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi
    A, value = smooth_noise()
    ctx = _ffi.Context(0)
    try:
        ctx.slab4d_begin(A.shape)
        ctx.set_origin4d(0, 0, 0, 0)
        ctx.upload_grid4d(np.ascontiguousarray(A[0:21]))
        ctx.extract4d(value, 1)
        with pytest.raises(_ffi.CxError):
            ctx.slab4d_append(20, 20)                     # not where the assembly stands (plane 0)
        with pytest.raises(_ffi.CxError):
            ctx.postprocess4d(100)                        # an assembly is open
        c = ctx.slab4d_append(0, 20)
        assert c["n_slabs"] == 1 and c["pending"] > 0
        with pytest.raises(_ffi.CxError):
            ctx.slab4d_finish(100)                        # planes 20..40 missing, halo references pending
        ctx.set_origin4d(20, 0, 0, 0)
        ctx.upload_grid4d(np.ascontiguousarray(A[20:40]))
        ctx.extract4d(value, 1)
        c = ctx.slab4d_append(20, 20)
        assert c["pending"] == 0 and c["n_slabs"] == 2
        post = ctx.slab4d_finish(100)
        keys = ctx.slab4d_keys(post)
        assert len(keys) == post["n_vertices"] and np.all(np.diff(keys) > 0)
        ctx.extract4d(value, 1)                           # a new extraction: the assembled result is gone
        with pytest.raises(_ffi.CxError):
            ctx.slab4d_keys(post)
        with pytest.raises(_ffi.CxError):
            ctx.morph_triangles()
    finally:
        ctx.set_origin4d(0, 0, 0, 0)
        ctx.close()


def _two_moving_balls(shape, dev, torch):
    "f = distance to the nearer of two balls minus its radius (fp32); the centres move 4 voxels over the time axis"
    n0, n1, n2, n3 = shape
    t = torch.arange(n3, dtype=torch.float32, device=dev) / (n3 - 1)
    c1 = (0.30 * n0 + 4.0 * t, 0.45 * n1 + 0.0 * t, 0.50 * n2 + 0.0 * t)
    c2 = (0.70 * n0 - 4.0 * t, 0.55 * n1 + 0.0 * t, 0.48 * n2 + 0.0 * t)
    r1, r2 = 0.16 * min(shape), 0.12 * min(shape)
    x = torch.arange(n0, dtype=torch.float32, device=dev)[:, None, None, None]
    y = torch.arange(n1, dtype=torch.float32, device=dev)[None, :, None, None]
    z = torch.arange(n2, dtype=torch.float32, device=dev)[None, None, :, None]
    d1 = torch.sqrt((x - c1[0]) ** 2 + (y - c1[1]) ** 2 + (z - c1[2]) ** 2) - r1
    d2 = torch.sqrt((x - c2[0]) ** 2 + (y - c2[1]) ** 2 + (z - c2[2]) ** 2) - r2
    A = torch.minimum(d1, d2).contiguous()
    del d1, d2
    centres = lambda tg: ((0.30 * n0 + 4.0 * tg / (n3 - 1), 0.45 * n1, 0.50 * n2), r1, (0.70 * n0 - 4.0 * tg / (n3 - 1), 0.55 * n1, 0.48 * n2), r2)
    return A, centres


def test_beyond_the_limit_on_the_device():
    """136 x 128 x 128 x 128 fp32 (> 2^28 samples) resident on the GPU, two moving balls: the slab path gives unique global edge ids,
    tetrahedra inside the assembly, consistently wound surfaces on the balls, and the same result in a different number of slabs"""
    torch = pytest.importorskip("torch")
    from contourist_amd import pentatopes
    from test_gpu_fullsize import edge_consistency
    shape = (136, 128, 128, 128)
    assert shape[0] * shape[1] * shape[2] * shape[3] > (1 << 28)
    A, centres = _two_moving_balls(shape, torch.device("cuda", 0), torch)
    try:
        m = pentatopes.GridContour4D(tuple(n - 1 for n in shape), A, 0.0)
        assert m._in_slabs()
        ft = m.find_tetrahedra()
        keys, pts, tets = ft["keys"], ft["points4d"], ft["tetrahedra"]
        assert m._slab_counts["n_slabs"] >= 2
        assert len(keys) == len(np.unique(keys)) == len(pts) and keys.dtype == np.int64
        assert len(tets) > 100000 and tets.min() >= 0 and tets.max() < len(pts)
        m.collect_morph_triangles()
        tmin, tmax = float(pts[:, 3].min()), float(pts[:, 3].max())
        times = [tmin + f * (tmax - tmin) for f in (0.13, 0.37, 0.52, 0.81)]
        for tg, (p, q) in zip(times, m.triangles_at_many(times)):
            manifold, same, other = edge_consistency(q)
            assert len(q) > 10000 and same == 0 and manifold > 1.3 * len(q)
            c1, r1, c2, r2 = centres(tg)
            d = np.minimum(np.abs(np.linalg.norm(p - np.array(c1), axis=1) - r1), np.abs(np.linalg.norm(p - np.array(c2), axis=1) - r2))
            assert d.max() < 0.25
        ncomp = m.n_components
        m.context().close()
        # the same volume in more slabs
        m2 = pentatopes.GridContour4D(tuple(n - 1 for n in shape), A, 0.0)
        m2.MAX_SAMPLES_PER_EXTRACTION = 1 << 27
        ft2 = m2.find_tetrahedra()
        assert m2._slab_counts["n_slabs"] > m._slab_counts["n_slabs"]
        assert np.array_equal(ft2["keys"], keys) and np.array_equal(ft2["points4d"].view(np.int64), pts.view(np.int64))
        assert ft2["counts"] == ft["counts"]
        assert np.array_equal(_canon_tets(keys, tets), _canon_tets(ft2["keys"], ft2["tetrahedra"]))
        m2.collect_morph_triangles()
        assert m2.n_components == ncomp
        m2.context().close()
    finally:
        del A
        torch.cuda.empty_cache()
