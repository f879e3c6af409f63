"""GPU: 3-D grids of 8- and 16-bit samples marched as they are.  Every result must equal, bit for bit, the same call on the
fp32 copy of the samples (samples.astype(float32); bfloat16: tensor.float()) on a context that holds only that fp32 grid."""
import numpy as np
import pytest

from contourist_amd import _ffi, synthetic, tetrahedral
from oracle import level0 as oracle_level0

pytestmark = pytest.mark.gpu

TYPES = ("uint8", "int8", "uint16", "int16", "float16", "bfloat16")
FLAG_SETS = (_ffi.CX_DIAG_CPYTHON310, _ffi.CX_DIAG_CANONICAL, _ffi.CX_DIAG_CPYTHON310 | _ffi.CX_KERNEL_GENERIC,
             _ffi.CX_DIAG_CPYTHON310 | _ffi.CX_KERNEL_FUSED, _ffi.CX_DIAG_CANONICAL | _ffi.CX_KERNEL_TILED)
SHAPES = ((40, 36, 64), (33, 29, 37), (24, 22, 3))    # aligned rows, ragged rows, rows shorter than 4 (the generic kernel)


def _torch():
    return pytest.importorskip("torch")


def _quantise(y, name):
    """a smooth fp32 field rounded into the range of a sample type: (typed array -- numpy, or a CPU torch tensor for bfloat16 --,
    its exact fp32 copy)"""
    y = np.asarray(y, dtype=np.float64)
    y = (y - y.min()) / (y.max() - y.min())
    if name in ("float16", "bfloat16"):
        x = (y - 0.5) * 40.0
        if name == "float16":
            q = x.astype(np.float16)
            return q, q.astype(np.float32)
        torch = _torch()
        q = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16)
        return q, q.float().numpy()
    info = np.iinfo(np.dtype(name))
    lo, hi = float(info.min) + 1, float(info.max) - 1
    q = np.clip(np.rint(lo + y * (hi - lo)), info.min, info.max).astype(name)
    return q, q.astype(np.float32)


def _field(shape, name, seed=5):
    if shape[2] < 4:     # (the generator sets two planes at each end of every axis to its minimum: rows of 3 from the middle of 8)
        y = synthetic.smooth_noise_numpy((shape[0], shape[1], 8), seed, passes=12)[:, :, 2:2 + shape[2]]
        return _quantise(np.ascontiguousarray(y), name)
    return _quantise(synthetic.smooth_noise_numpy(shape, seed, passes=12), name)


def _isovalues(f32):
    """one isovalue equal to many samples (the tolerance rules of the reference), one halfway between two representable values"""
    vals, counts = np.unique(f32, return_counts=True)
    mid = len(vals) // 2
    common = vals[max(range(mid - len(vals) // 8, mid + len(vals) // 8 + 1), key=lambda i: counts[i])]
    return float(common), 0.5 * (float(vals[mid]) + float(vals[mid + 1]))


def _bind(ctx, q, device_offset=False):
    """bind the typed samples: numpy -> upload in their type; bfloat16, or device_offset -> a device tensor (at an offset of one
    element: the unaligned kernels)"""
    if isinstance(q, np.ndarray) and not device_offset:
        ctx.upload_grid_native(q)
        return None
    torch = _torch()
    t = q if not isinstance(q, np.ndarray) else torch.from_numpy(q)
    if device_offset:
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
        flat[1:] = t.reshape(-1).cuda()
        d = flat[1:].view(t.shape)
    else:
        d = t.cuda().contiguous()
    ctx.adopt_device_grid(d.data_ptr(), tuple(d.shape), keepalive=d, dtype=d.dtype)
    return d


def _level0(ctx, value, flags):
    c = ctx.extract3d(value, flags)
    keys, t, tris = ctx.download_level0_records(c)
    xyz, keys2, tris2 = ctx.download_level0(c)
    return dict(counts=c, keys=keys, tbits=t.view(np.uint32).copy(), tris=tris, xyz=xyz, path=ctx.level0_path())


def _canonical(L):
    return oracle_level0.canonical_level0(L["keys"].astype(np.int64), L["xyz"].view(np.uint32), L["tris"].astype(np.int64))


def _assert_same_level0(a, b, exact_order):
    assert a["counts"] == b["counts"]
    ca, cb = _canonical(a), _canonical(b)
    for x, y in zip(ca, cb):
        assert np.array_equal(x, y)
    if exact_order:
        assert np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["tbits"], b["tbits"]) and np.array_equal(a["tris"], b["tris"])


@pytest.mark.parametrize("name", TYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_level0_equals_fp32(name, shape):
    q, f32 = _field(shape, name)
    typed, plain = _ffi.Context(0), _ffi.Context(0)
    plain.upload_grid(f32)
    binds = [False, True] if shape[2] >= 4 else [False]
    for device_offset in binds:
        keep = _bind(typed, q, device_offset)
        info = typed.grid_info()
        assert info["dtype"] == name
        common, halfway = _isovalues(f32)
        for value in (common, halfway):
            for flags in FLAG_SETS:
                a, b = _level0(typed, value, flags), _level0(plain, value, flags)
                assert a["counts"]["n_triangles"] > 0
                assert a["path"] in (0, 1)                       # typed grids: the fused / tile requests run the staged kernels
                # the staged kernels number the records the same way every run unless waves take the tolerance path (an isovalue
                # equal to samples) -- there, and for the generic kernel's atomics, the comparison is the canonical one
                _assert_same_level0(a, b, exact_order=(a["path"] == b["path"] == 1 and value == halfway))
        del keep


@pytest.mark.parametrize("name", TYPES)
def test_grid_info_reports_the_typed_bytes(name):
    q, f32 = _field((20, 18, 16), name)
    ctx = _ffi.Context(0)
    n = f32.size
    if isinstance(q, np.ndarray):
        ctx.upload_grid_native(q)
        assert ctx.grid_info() == dict(dtype=name, device_bytes=n * q.dtype.itemsize)
    d = _bind(ctx, q, device_offset=True)
    assert ctx.grid_info() == dict(dtype=name, device_bytes=0)       # adopted: the context holds nothing of its own
    ctx.upload_grid(f32)
    assert ctx.grid_info() == dict(dtype="float32", device_bytes=n * 4)
    del d


@pytest.mark.parametrize("name", TYPES)
def test_points_and_triangles_equal_fp32(name):
    torch = _torch()
    q, f32 = _field((34, 30, 40), name, seed=11)
    value = _isovalues(f32)[1]
    mins, maxes, delta = [-1.0, 0.5, 2.0], [0.0, 0.0, 0.0], [0.25, 0.5, 0.125]
    arr = q if isinstance(q, np.ndarray) else q.cuda()
    S = tetrahedral.TriangulatedIsosurfaces(mins, maxes, delta, arr, value, [])
    R = tetrahedral.TriangulatedIsosurfaces(mins, maxes, delta, f32, value, [])
    p, t = S.get_points_and_triangles()
    pr, tr = R.get_points_and_triangles()
    assert len(tr) > 0
    assert np.array_equal(np.asarray(p, dtype=np.float64), np.asarray(pr, dtype=np.float64)) and np.array_equal(np.asarray(t), np.asarray(tr))
    S2 = tetrahedral.TriangulatedIsosurfaces(mins, maxes, delta, arr, value, [])
    R2 = tetrahedral.TriangulatedIsosurfaces(mins, maxes, delta, f32, value, [])
    pd, td = S2.get_points_and_triangles(device=True)
    prd, trd = R2.get_points_and_triangles(device=True)
    assert torch.equal(torch.as_tensor(pd).cpu(), torch.as_tensor(prd).cpu()) and torch.equal(torch.as_tensor(td).cpu(), torch.as_tensor(trd).cpu())


@pytest.mark.parametrize("name", TYPES)
def test_device_tensor_is_accepted(name):
    """a torch tensor of the type on the GPU: GridContour3d binds it as it is (the fp32-only assert refused it)"""
    torch = _torch()
    q, f32 = _field((26, 24, 28), name, seed=2)
    d = (torch.from_numpy(q) if isinstance(q, np.ndarray) else q).cuda()
    value = _isovalues(f32)[1]
    corner = tuple(n - 1 for n in f32.shape)
    m = tetrahedral.GridContour3d(corner, d, value)
    r = tetrahedral.GridContour3d(corner, f32, value)
    p, t = m.get_points_and_triangles()
    pr, tr = r.get_points_and_triangles()
    assert m.context().grid_info()["dtype"] == name
    assert len(tr) > 0 and np.array_equal(np.asarray(p), np.asarray(pr)) and np.array_equal(np.asarray(t), np.asarray(tr))


@pytest.mark.parametrize("name", TYPES)
def test_levels_equal_fp32(name):
    q, f32 = _field((36, 32, 44), name, seed=8)
    vals = np.unique(f32)
    picks = [float(vals[int(i)]) for i in np.linspace(len(vals) * 0.2, len(vals) * 0.8, 4)]
    values = picks + [0.5 * (float(vals[int(i)]) + float(vals[int(i) + 1])) for i in np.linspace(len(vals) * 0.25, len(vals) * 0.75, 4)]
    typed, plain = _ffi.Context(0), _ffi.Context(0)
    keep = _bind(typed, q)
    plain.upload_grid(f32)
    ca, cb = typed.extract3d_levels(values), plain.extract3d_levels(values)
    assert ca == cb and len(ca) == 8
    for i in range(8):
        typed.select_level(i)
        plain.select_level(i)
        a, b = typed.download_level0_records(ca[i]), plain.download_level0_records(cb[i])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
    # and through the public class
    arr = q if isinstance(q, np.ndarray) else q.cuda()
    A = list(tetrahedral.MultiLevelIsosurfaces([0.0] * 3, [1.0] * 3, [0.5] * 3, arr, values[:3]).levels())
    B = list(tetrahedral.MultiLevelIsosurfaces([0.0] * 3, [1.0] * 3, [0.5] * 3, f32, values[:3]).levels())
    for (va, pa, ta), (vb, pb, tb) in zip(A, B):
        assert va == vb and np.array_equal(np.asarray(pa), np.asarray(pb)) and np.array_equal(np.asarray(ta), np.asarray(tb))
    del keep


@pytest.mark.parametrize("name", TYPES)
def test_seeded_selection_equals_fp32(name):
    q, f32 = _field((30, 28, 32), name, seed=4)
    value = _isovalues(f32)[1]
    typed, plain = _ffi.Context(0), _ffi.Context(0)
    keep = _bind(typed, q)
    plain.upload_grid(f32)
    ca, cb = typed.extract3d(value), plain.extract3d(value)
    keys, _t, _tris = plain.download_level0_records(cb)
    lo, hi = tetrahedral.unpack_edge_ids(keys[:: max(1, len(keys) // 5)][:5], f32.shape)
    eps = [(tuple(int(x) for x in a), tuple(int(x) for x in b)) for a, b in zip(lo, hi)]
    for parallel in (False, True):
        sa, sb = typed.select_seeded(eps, parallel=parallel), plain.select_seeded(eps, parallel=parallel)
        assert sa == sb and sa["triangles_kept"] > 0
        ma, mb = typed.seeded_masks(ca), plain.seeded_masks(cb)
        assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1], mb[1])
    pa, pb = typed.postprocess3d(), plain.postprocess3d()
    assert pa == pb
    La, Lb = typed.download_level1(pa), plain.download_level1(pb)
    for x, y in zip(La, Lb):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    del keep


def test_rebinding_fp32_after_a_typed_grid():
    """a typed grid, then cx_grid_upload on the same context: fp32 again (the owned buffer is reused by bytes), result == a fresh context's"""
    q, f32 = _field((40, 36, 64), "uint8")
    q16, f16 = _field((40, 36, 64), "int16", seed=9)
    big, big32 = _field((48, 40, 64), "uint16", seed=6)
    ctx = _ffi.Context(0)
    ctx.upload_grid_native(q)
    ctx.extract3d(_isovalues(f32)[1])
    ctx.upload_grid_native(big)           # grows the owned buffer past the uint8 grid's bytes
    ctx.extract3d(_isovalues(big32)[1])
    for arr, ref in ((f16, None), (q16, f16)):
        if ref is None:
            ctx.upload_grid(arr)
            assert ctx.grid_info()["dtype"] == "float32"
        else:
            ctx.upload_grid_native(arr)
            assert ctx.grid_info()["dtype"] == "int16"
        fresh = _ffi.Context(0)
        fresh.upload_grid(f16)
        v = _isovalues(f16)[1]
        _assert_same_level0(_level0(ctx, v, _ffi.CX_DIAG_CPYTHON310), _level0(fresh, v, _ffi.CX_DIAG_CPYTHON310), exact_order=True)


def test_4d_paths_unchanged():
    """4-D stays fp32: a typed numpy array is widened and marched as before (same counts as its fp32 copy); a typed torch tensor
    is refused as before"""
    torch = _torch()
    from contourist_amd import pentatopes
    rng = np.random.RandomState(1)
    A = np.rint(rng.standard_normal((6, 7, 6, 5)) * 50).astype(np.int16)
    corner = tuple(n - 1 for n in A.shape)
    a = pentatopes.GridContour4D(corner, A, 0.5)
    b = pentatopes.GridContour4D(corner, A.astype(np.float32), 0.5)
    ma, mb = a.march(), b.march()
    assert ma["counts"] == mb["counts"] and len(mb["keys"]) > 0
    for k in ("xyzt", "keys", "tetrahedra"):
        assert np.array_equal(np.asarray(ma[k]), np.asarray(mb[k]))
    with pytest.raises(AssertionError) as e:      # the march's check has no message, as before
        pentatopes.GridContour4D(corner, torch.from_numpy(A).cuda(), 0.5).march()
    assert str(e.value) == ""
    s = pentatopes.GridContour4D(corner, torch.from_numpy(A).cuda(), 0.5)
    s.MAX_SAMPLES_PER_EXTRACTION = 7 * 6 * 5 * 3
    assert s._in_slabs()
    with pytest.raises(AssertionError, match="^device samples must be a contiguous float32 tensor on the GPU$"):
        s.find_tetrahedra()


@pytest.mark.parametrize("name", ("int16", "uint8"))
def test_bench_field_at_full_size(name):
    """the 512^3 bench field (smooth_noise_host, seed 1235, 1400 passes: what bench.py extracts) quantised to the type as
    tools/bench_dtype.py does it: the whole-volume Level 0 equals the fp32 run's on the same values"""
    y = synthetic.smooth_noise_host((512, 512, 512), 1235, 1400)
    if name == "int16":
        q = np.rint(y * (30000.0 / float(np.abs(y).max()))).astype(np.int16)
        value = 0.5
    else:
        lo, hi = float(y.min()), float(y.max())
        q = np.rint((y - lo) / (hi - lo) * 254.0).astype(np.uint8)
        value = float(np.floor(-lo / (hi - lo) * 254.0)) + 0.5
    del y
    f32 = q.astype(np.float32)
    typed, plain = _ffi.Context(0), _ffi.Context(0)
    typed.upload_grid_native(q)
    assert typed.grid_info() == dict(dtype=name, device_bytes=q.size * q.dtype.itemsize)
    plain.upload_grid(f32)
    for flags in (_ffi.CX_DIAG_CPYTHON310, _ffi.CX_DIAG_CANONICAL):
        a, b = _level0(typed, value, flags), _level0(plain, value, flags)
        assert a["counts"]["n_triangles"] > 1000000
        _assert_same_level0(a, b, exact_order=True)


def _rows_with_winding(tris):
    "triangles as rows rotated to start at their smallest index (winding kept), rows sorted: the triangle set, any order"
    T = np.asarray(tris, dtype=np.int64)
    r = np.argmin(T, axis=1)
    T = np.stack([T[np.arange(len(T)), (r + s) % 3] for s in range(3)], axis=1)
    return T[np.lexsort((T[:, 2], T[:, 1], T[:, 0]))]


def test_uint16_volume_beyond_one_extraction():
    """1056 x 720 x 720 uint16 = 547 M samples (> 2^29, 1.1 GB) on the GPU: marched in slabs in its own type, the Level-1 mesh equals
    the fp32 slab run's on the same values (points in ascending edge id; triangles as a set, windings included)"""
    torch = _torch()
    shape = (1056, 720, 720)
    assert shape[0] * shape[1] * shape[2] > (1 << 29)
    ax = [torch.arange(n, dtype=torch.float32, device="cuda") for n in shape]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    c1, r1 = (0.30 * shape[0], 0.45 * shape[1], 0.50 * shape[2]), 0.18 * min(shape)
    c2, r2 = (0.72 * shape[0], 0.55 * shape[1], 0.48 * shape[2]), 0.13 * min(shape)
    d = torch.minimum(torch.sqrt((X - c1[0]) ** 2 + (Y - c1[1]) ** 2 + (Z - c1[2]) ** 2) - r1,
                      torch.sqrt((X - c2[0]) ** 2 + (Y - c2[1]) ** 2 + (Z - c2[2]) ** 2) - r2)
    del X, Y, Z
    qi = torch.clamp(torch.round(d * 16.0) + 32768.0, 0.0, 65535.0).to(torch.int32)
    del d
    q = qi.to(torch.uint16).contiguous()
    f32 = qi.to(torch.float32).contiguous()
    del qi
    value = 32768.5
    corner = tuple(n - 1 for n in shape)
    res = []
    for S in (q, f32):
        m = tetrahedral.GridContour3d(corner, S, value)
        assert m._in_slabs()
        p, t = m.get_points_and_triangles()
        assert m._slab_counts["n_slabs"] >= 2 and m._post["n_components"] == 2
        res.append((np.asarray(p), np.asarray(t), m.context().grid_info()["dtype"]))
        del m
    assert res[0][2] == "uint16" and res[1][2] == "float32"
    assert len(res[1][1]) > 2000000
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(_rows_with_winding(res[0][1]), _rows_with_winding(res[1][1]))


def test_big_endian_samples():
    """a big-endian volume ('>i2', '>u2', '>f2': np.fromfile, FITS) is read by its values, not its raw bytes: the typed paths give
    what its fp32 copy gives"""
    for name in ("int16", "uint16", "float16"):
        q, f32 = _field((30, 28, 32), name, seed=12)
        big = q.astype(q.dtype.newbyteorder(">"))
        assert not big.dtype.isnative and np.array_equal(big.astype(np.float32), f32)
        value = _isovalues(f32)[1]
        typed, plain = _ffi.Context(0), _ffi.Context(0)
        typed.upload_grid_native(big)
        assert typed.grid_info()["dtype"] == name
        plain.upload_grid(f32)
        _assert_same_level0(_level0(typed, value, _ffi.CX_DIAG_CPYTHON310), _level0(plain, value, _ffi.CX_DIAG_CPYTHON310), exact_order=True)
        mins, delta = [0.0, 0.0, 0.0], [0.5, 0.5, 0.5]
        p, t = tetrahedral.TriangulatedIsosurfaces(mins, [1.0] * 3, delta, big, value, []).get_points_and_triangles()
        pr, tr = tetrahedral.TriangulatedIsosurfaces(mins, [1.0] * 3, delta, f32, value, []).get_points_and_triangles()
        assert len(tr) > 0 and np.array_equal(np.asarray(p), np.asarray(pr)) and np.array_equal(np.asarray(t), np.asarray(tr))


def test_uint16_volume_in_slabs():
    """a uint16 volume through the slab path (limit lowered, as tests/test_gpu_fullsize.py does): Level 1 equals the fp32 slab run's"""
    torch = _torch()
    q, f32 = _field((70, 48, 52), "uint16", seed=77)
    value = _isovalues(f32)[1]
    corner = tuple(n - 1 for n in f32.shape)
    for limit, on_device in ((48 * 52 * 16, False), (48 * 52 * 24, True)):
        res = []
        for arr in (q, f32):
            S = torch.from_numpy(arr).cuda() if on_device else arr
            m = tetrahedral.GridContour3d(corner, S, value)
            m.MAX_SAMPLES_PER_EXTRACTION = limit
            assert m._in_slabs()
            p, t = m.get_points_and_triangles()
            assert m._slab_counts["n_slabs"] >= 2
            res.append((np.asarray(p), np.asarray(t), m.context().grid_info()["dtype"]))
        assert res[0][2] == "uint16" and res[1][2] == "float32"
        assert len(res[1][1]) > 1000
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
