"""cx_grid_distance3d (csrc/cx_dist.hip) against its numpy restatement (tests/distance_ref.py), bit for bit: shapes around the kernels'
tiles (a wave owns a row in the first kernel and 64 columns of one position of the walked axis in the second), site patterns from dense
to a single corner, three sides, three output kinds, unit and anisotropic sampling, every sample type from the host and from a device
tensor, NaN and infinite samples, misaligned slices of a caller's output, contourist_amd.volume, the end-to-end routes
uint8 -> signed distance -> bind -> march and uint8 -> dilate -> bind -> march with no float array on the host, what a call leaves alone
and what a bind resets, and the error codes."""
import os

import numpy as np
import pytest

import distance_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

STRADDLE = (37, 33, 259)      # 2 x 16 + 5 planes, 2 x 16 + 1 rows, 4 x 64 + 3 columns
SAMPLINGS = [None, (2.5, 1.0, 0.7), (0.3, 0.3, 1.25)]
KIND_DTYPE = {"squared": np.float64, "float32": np.float32, "mask": np.uint8}


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def same(got, want):
    "bit for bit (the results hold no NaN: an infinity has one pattern)"
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    view = {8: np.uint64, 4: np.uint32, 1: np.uint8}[got.dtype.itemsize]
    bad = got.view(view) != want.view(view)
    assert not bad.any(), (int(bad.sum()), got[bad][:4], want[bad][:4])


def radii2(parts):
    "0, 1, 2.25 and a squared distance that occurs in the field (the smallest finite one above 2.25, else the largest finite one)"
    finite = np.concatenate([p[np.isfinite(p)] for p in parts])
    above = finite[finite > 2.25]
    return [0.0, 1.0, 2.25, float(above.min() if len(above) else finite.max())]


def check_all(ctx, A, value, samplings=SAMPLINGS, samples=None, as_values=None):
    """every side and kind of the device transform of host samples A (or of `samples`, whose values are `as_values`) == the restatement"""
    V = A if as_values is None else as_values
    src = A if samples is None else samples
    for sampling in samplings:
        parts = R.both(V, value, sampling)
        for side in R.SIDES:
            n, got = ctx.distance_grid(value, side, "squared", sampling, samples=src, download=True)
            assert n == R.n_sites(V, value, side)
            same(got, R.squared(V, value, side, parts=parts))
            n, got = ctx.distance_grid(value, side, "float32", sampling, samples=src, download=True)
            assert n == R.n_sites(V, value, side)
            same(got, R.distance(V, value, side, parts=parts))
            if side != "signed":
                for r2 in radii2(parts):
                    _, got = ctx.distance_grid(value, side, "mask", sampling, r2, samples=src, download=True)
                    same(got, R.mask(V, value, side, r2, parts=parts))


def uniform(shape, seed):
    return np.random.RandomState(seed).uniform(size=shape).astype(np.float32)


SHAPES = [(1, 1, 1), (2, 2, 2), (1, 8, 9), (5, 4, 3), (3, 5, 63), (3, 5, 64), (2, 6, 65), (2, 3, 131), STRADDLE]


@pytest.mark.parametrize("density", [0.5, 0.03, 0.001])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_sites(ctx, shape, density):
    "the samples that are not low (the sites of 'below') have this density; the low ones are the sparse side at 1 - density"
    A = uniform(shape, 11)
    check_all(ctx, A, 1.0 - density)
    if shape == STRADDLE:
        check_all(ctx, A, density, samplings=[None])      # sparse low samples: the long searches are those of 'above'


def test_one_site_in_a_corner(ctx):
    "scans longer than a wave's row of 64 and than any window: every sample's search runs to the corner, and most rows have no site"
    A = np.zeros((40, 40, 70), dtype=np.float32)
    A[39, 0, 69] = 1.0
    check_all(ctx, A, 0.5, samplings=[None, (0.3, 0.3, 1.25)])
    _, got = ctx.distance_grid(0.5, "below", "squared", samples=A, download=True)
    assert got[0, 39, 0] == 39 ** 2 + 39 ** 2 + 69 ** 2


def test_one_full_plane(ctx):
    for axis in range(3):
        A = np.zeros((9, 10, 70), dtype=np.float32)
        index = [slice(None)] * 3
        index[axis] = 3
        A[tuple(index)] = 1.0
        check_all(ctx, A, 0.5, samplings=[None, (2.5, 1.0, 0.7)])


def test_checkerboard(ctx):
    "ties everywhere: a minimum has one value whichever candidate gives it"
    i, j, k = np.meshgrid(np.arange(7), np.arange(6), np.arange(67), indexing="ij")
    check_all(ctx, ((i + j + k) % 2).astype(np.float32), 0.5)
    check_all(ctx, ((i // 2 + j // 3 + k // 5) % 2).astype(np.uint8), 0.5, samplings=[None])


def test_no_site_and_all_sites(ctx):
    from contourist_amd import _ffi
    A = uniform((5, 6, 70), 12)
    check_all(ctx, A, -1.0, samplings=[None, (2.5, 1.0, 0.7)])      # nothing is low: 'above' has no site
    check_all(ctx, A, 2.0, samplings=[None])                        # everything is low: 'below' has none
    n, got = ctx.distance_grid(2.0, "below", "float32", samples=A, download=True)
    assert n == 0 and np.all(np.isposinf(got))
    n, got = ctx.distance_grid(2.0, "above", "float32", samples=A, download=True)
    assert n == A.size and not got.any()
    n, got = ctx.distance_grid(2.0, "below", "mask", None, 1e300, samples=A, download=True)
    assert n == 0 and not got.any()
    # an infinite result is not bound and stays pending
    for side in ("below", "signed"):
        n, ptr = ctx.distance_grid(2.0, side, "float32", samples=A)
        assert n == 0
        with pytest.raises(_ffi.CxError) as e:
            ctx.bind_distance()
        assert e.value.code == _ffi.CX_ERR_INVALID
        assert ctx.distance_result() == (A.shape, ptr, "float32", 0)


@pytest.mark.parametrize("name", ["float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16"])
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    shape = (7, 18, 67)
    rng = np.random.RandomState(9)
    if name == "bfloat16":
        t = torch.from_numpy((rng.standard_normal(shape) * 3.0).astype(np.float32)).cuda().to(torch.bfloat16)
        values = t.float().cpu().numpy()
        host = (t.view(torch.int16).cpu().numpy().view(np.uint16), "bfloat16", shape)
        value = 1.3
    elif np.dtype(name).kind == "f":
        values = (rng.standard_normal(shape) * 3.0).astype(name)
        t, host, value = torch.from_numpy(values).cuda(), values, 1.3
    else:
        info = np.iinfo(name)
        values = rng.randint(info.min, info.max + 1, size=shape).astype(name)
        values[0, 0, :2] = [info.min, info.max]
        t, host = torch.from_numpy(values).cuda(), values
        value = info.min + 0.8 * (float(info.max) - float(info.min)) + 0.5
    torch.cuda.synchronize()
    check_all(ctx, values, value, samplings=[None, (2.5, 1.0, 0.7)], samples=host, as_values=values)
    check_all(ctx, values, value, samplings=[None], samples=(t.data_ptr(), t.dtype, shape), as_values=values)
    if name not in ("float32", "bfloat16", "float16"):      # a value that is a sample value: f < value is strict
        check_all(ctx, values, float(values[3, 3, 3]), samplings=[None], samples=host, as_values=values)


def test_the_low_rule_on_the_device(ctx):
    "NaN, infinities, -0.0 against 0.0 and a value between two float32 neighbours"
    A = uniform((4, 5, 70), 13) - 0.5
    A[1, 2, 3], A[2, 3, 60], A[3, 1, 33], A[0, 0, 0], A[0, 0, 1] = np.nan, np.inf, -np.inf, -0.0, 0.0
    A[1] = np.where(A[1] < 0, np.float32(-0.0), np.float32(0.0))
    A[1, 2, 3] = np.nan
    for value in (0.0, -0.0, 5e-324, 0.1):
        check_all(ctx, A, value, samplings=[None])
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(2.0))
    B = np.where(uniform((3, 4, 66), 14) < 0.5, a, b).astype(np.float32)
    for value in ((np.float64(a) + np.float64(b)) / 2, np.float64(b), np.nextafter(np.float64(a), 2.0)):
        assert 0 < R.n_sites(B, value, "below") < B.size
        check_all(ctx, B, value, samplings=[None])


def test_misaligned_slices_and_callers_output(ctx):
    import torch
    from contourist_amd import _ffi
    shape = (5, 9, 71)
    n = int(np.prod(shape))
    torch_types = {"squared": torch.float64, "float32": torch.float32, "mask": torch.uint8}
    for np_dtype, off in ((np.float32, 1), (np.uint8, 1), (np.int16, 3), (np.uint8, 7)):
        rng = np.random.RandomState(off + 20)
        flat = (rng.uniform(size=n + off) * 100).astype(np_dtype)
        t = torch.from_numpy(flat).cuda()[off:]
        assert t.data_ptr() % 16 != 0
        A = flat[off:].reshape(shape)
        parts = R.both(A, 70.5, (2.5, 1.0, 0.7))
        for kind, side in (("squared", "signed"), ("float32", "signed"), ("mask", "below")):
            want = R.squared(A, 70.5, side, parts=parts) if kind == "squared" else R.distance(A, 70.5, side, parts=parts) if kind == "float32" \
                else R.mask(A, 70.5, side, 2.25, parts=parts)
            guard = 7 if kind == "mask" else -7.0
            for lead in (1, 3):      # elements in front: the slice is aligned to its own type and to nothing more
                out = torch.full((n + lead + 2,), guard, dtype=torch_types[kind], device="cuda")
                torch.cuda.synchronize()
                sites, ptr = ctx.distance_grid(70.5, side, kind, (2.5, 1.0, 0.7), 2.25, samples=(t.data_ptr(), t.dtype, shape), out=out[lead:].data_ptr())
                host = out.cpu().numpy()
                assert sites == R.n_sites(A, 70.5, side) and ptr == out[lead:].data_ptr()
                assert np.all(host[:lead] == guard) and np.all(host[lead + n:] == guard)      # nothing written around the result
                same(host[lead:lead + n].reshape(shape), want)
                with pytest.raises(_ffi.CxError) as e:      # with an output of the caller's the context holds no result
                    ctx.distance_result()
                assert e.value.code == _ffi.CX_ERR_STATE


def test_two_calls_give_the_same_bits(ctx):
    A = uniform(STRADDLE, 17)
    a = ctx.distance_grid(0.97, "signed", "squared", (0.3, 0.3, 1.25), samples=A, download=True)[1]
    ctx.distance_grid(0.5, "below", "mask", None, 1.0, samples=uniform((3, 3, 3), 1), download=True)      # (the scratch is reused in between)
    b = ctx.distance_grid(0.97, "signed", "squared", (0.3, 0.3, 1.25), samples=A, download=True)[1]
    same(a, b)


def quantised_noise():
    A = np.load(os.path.join(GOLDEN_DIR, "noise32_v0.npz"))["A"]
    lo, hi = float(A.min()), float(A.max())
    return np.clip(np.rint((A - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)


def march_both_routes(U, device_route, host_grid, value):
    "the Level-0 mesh of the grid `device_route(context)` leaves bound == that of `host_grid` uploaded"
    from contourist_amd import _ffi
    meshes = []
    for route in ("device", "host"):
        c = _ffi.Context()
        try:
            if route == "device":
                c.upload_grid_native(U)
                assert c.grid_info() == dict(dtype="uint8", device_bytes=U.size)
                device_route(c)
                assert c.shape == U.shape
            else:
                c.upload_grid_native(host_grid)
            assert c.grid_info() == dict(dtype=host_grid.dtype.name, device_bytes=host_grid.nbytes)
            counts = c.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
            meshes.append((counts, c.download_level0_records(counts)))
        finally:
            c.close()
    (c0, m0), (c1, m1) = meshes
    assert c0 == c1 and c0["n_triangles"] > 1000
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1].view(np.uint32), m1[1].view(np.uint32)) and np.array_equal(m0[2], m1[2])


def test_upload_signed_distance_bind_march():
    "a uint8 volume is uploaded, turned into its signed distance field and marched at 0 with no float array on the host"
    U = quantised_noise()

    def route(c):
        n, ptr = c.distance_grid(127.3, "signed")      # the bound grid in, the context's own buffer out
        assert n == R.n_sites(U, 127.3, "signed") and c.distance_result() == (U.shape, ptr, "float32", n)
        c.bind_distance()

    march_both_routes(U, route, R.distance(U, 127.3, "signed"), 0.0)


def test_upload_dilate_bind_march():
    U = quantised_noise()

    def route(c):
        c.distance_grid(150.5, "below", "mask", radius2=4.0)
        c.bind_distance()

    march_both_routes(U, route, R.mask(U, 150.5, "below", 4.0), 0.5)


def test_volume_module(ctx):
    import torch
    from contourist_amd import volume
    A = uniform((20, 33, 70), 15)
    U = (uniform((20, 33, 70), 16) * 255).astype(np.uint8)
    for S, value in ((A, 0.9), (U, 230.5)):
        parts = R.both(S, value)
        for side in R.SIDES:
            same(volume.distance(S, value, side), R.distance(S, value, side, parts=parts))
            same(volume.distance(S, value, side, squared=True), R.squared(S, value, side, parts=parts))
        same(volume.signed_distance(S, value), R.distance(S, value, "signed", parts=parts))
        same(volume.signed_distance(S, value, sampling=(2.5, 1.0, 0.7)), R.distance(S, value, "signed", (2.5, 1.0, 0.7)))
        same(volume.distance(S, value, sampling=0.5), R.distance(S, value, "below", (0.5, 0.5, 0.5)))
        for radius in (1.0, 2.0):
            same(volume.dilate(S, value, radius), R.dilate(S, value, radius))
            same(volume.erode(S, 1.0 - value if S is A else 25.5, radius), R.erode(S, 1.0 - value if S is A else 25.5, radius))
    # open and close a small mask: specks go, pinholes close
    M = (uniform((12, 14, 40), 18) < 0.02).astype(np.uint8)
    M[3:9, 4:11, 6:30] = 1
    M[5, 7, 12] = 0
    for radius, sampling in ((1.0, None), (1.5, None), (2.0, (2.0, 1.0, 0.5))):
        o, c = volume.opened(M, 0.5, radius, sampling), volume.closed(M, 0.5, radius, sampling)
        same(o, R.opened(M, 0.5, radius, sampling))
        same(c, R.closed(M, 0.5, radius, sampling))
    assert volume.opened(M, 0.5, 1.0)[5, 7, 12] == 0 and volume.closed(M, 0.5, 1.0)[5, 7, 12] == 1
    assert volume.opened(M, 0.5, 1.0).sum() < M.sum()
    same(volume.dilate(M.astype(bool), 0.5, 1.0), R.dilate(M, 0.5, 1.0))
    # a tensor in, a tensor out
    t = torch.from_numpy(U).cuda()
    d = volume.signed_distance(t, 230.5)
    assert d.is_cuda and d.dtype == torch.float32
    same(d.cpu().numpy(), R.distance(U, 230.5, "signed"))
    d2 = volume.distance(t, 230.5, "above", squared=True)
    assert d2.dtype == torch.float64
    same(d2.cpu().numpy(), R.squared(U, 230.5, "above"))
    tm = torch.from_numpy(M).cuda()
    for fn, ref in ((volume.dilate, R.dilate), (volume.erode, R.erode), (volume.opened, R.opened), (volume.closed, R.closed)):
        got = fn(tm, 0.5, 1.5)
        assert got.is_cuda and got.dtype == torch.uint8
        same(got.cpu().numpy(), ref(M, 0.5, 1.5))
    # two dimensions and one; float64 samples are rounded to float32 first
    B = A[3]
    same(volume.distance(B, 0.9, sampling=(1.0, 0.7)), R.distance(B[None], 0.9, "below", (1.0, 1.0, 0.7))[0])
    same(volume.signed_distance(B[5], 0.9), R.distance(B[5][None, None], 0.9, "signed")[0, 0])
    same(volume.dilate(torch.from_numpy(B).cuda(), 0.9, 2.0).cpu().numpy(), R.dilate(B[None], 0.9, 2.0)[0])
    same(volume.distance(A.astype(np.float64) + 1e-12, 0.9), R.distance((A.astype(np.float64) + 1e-12).astype(np.float32), 0.9))


def test_a_call_leaves_the_state_and_binding_resets_it():
    from contourist_amd import _ffi
    A = np.random.RandomState(19).standard_normal((12, 13, 70)).astype(np.float32)
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        cap = c.cap3d()
        cap_mesh = c.download_cap(cap)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)                                                # a pending filter result
        c.distance_grid(0.1, "signed")                                            # of the bound grid, into the context
        c.distance_grid(0.5, "below", samples=np.zeros((5, 6, 7), dtype=np.uint8), download=True)      # of other samples
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert all(np.array_equal(a, b) for a, b in zip(cap_mesh, c.download_cap(cap)))
        assert c.filter_result() == filt
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts               # the grid is the one uploaded
        levels = c.extract3d_levels([-0.4, 0.1, 0.6], _ffi.CX_DIAG_CPYTHON310)
        c.select_level(1)
        sel = c.download_level0_records(levels[1])
        n, ptr = c.distance_grid(0.1, "signed")
        assert c.counts() == levels[1]
        assert all(np.array_equal(a, b) for a, b in zip(sel, c.download_level0_records(levels[1])))
        c.select_level(2)
        assert c.counts() == levels[2]
        cap = c.cap3d()
        p = c.postprocess3d()
        # a filter call does not disturb the pending distance result either
        filt = c.filter_grid(axes)
        assert c.distance_result() == (A.shape, ptr, "float32", n) and c.filter_result() == filt
        # bind: as after an upload; the filter's result stays
        c.bind_distance()
        for gone in (c.counts, lambda: c.select_level(0), lambda: c.download_level1(p), c.distance_result, c.bind_distance, lambda: c.download_cap(cap)):
            with pytest.raises(_ffi.CxError) as e:
                gone()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert c.filter_result() == filt
        assert c.shape == A.shape and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        again = c.extract3d(0.0, _ffi.CX_DIAG_CPYTHON310)
        fresh = _ffi.Context()
        try:
            fresh.upload_grid(R.distance(A, 0.1, "signed"))
            assert fresh.extract3d(0.0, _ffi.CX_DIAG_CPYTHON310) == again
        finally:
            fresh.close()
        # the bound grid transformed again, and bound again: the grid owned before is released
        live = _ffi.device_bytes(c.handle)[0]
        c.distance_grid(0.0, "signed")
        c.bind_distance()
        assert _ffi.device_bytes(c.handle)[0] == live
        # squared distances and a result the march does not take stay pending
        c.distance_grid(0.0, "signed", "squared")
        with pytest.raises(_ffi.CxError) as e:
            c.bind_distance()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.distance_result()[2] == "squared"
        thin = np.zeros((1, 13, 70), dtype=np.uint8)
        thin[0, 4, 5] = 1
        n, ptr = c.distance_grid(0.5, "signed", samples=thin)
        with pytest.raises(_ffi.CxError) as e:
            c.bind_distance()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.distance_result() == ((1, 13, 70), ptr, "float32", 1) and c.shape == A.shape
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import ctypes
    import torch
    from contourist_amd import _ffi
    A = uniform((4, 5, 6), 21)

    def code(value=0.5, side="below", kind="float32", sampling=None, radius2=0.0, samples=A, **kw):
        with pytest.raises(_ffi.CxError) as e:
            ctx.distance_grid(value, side, kind, sampling, radius2, samples=samples, **kw)
        return e.value.code

    fresh = _ffi.Context()
    try:
        for call in (lambda: fresh.distance_grid(0.5), fresh.distance_result, fresh.bind_distance):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    for value in (float("nan"), float("inf"), -float("inf")):
        assert code(value=value) == _ffi.CX_ERR_INVALID
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-170, 1e160):      # (the last two: the square is not a normal double)
        for axis in range(3):
            sampling = [1.0, 1.0, 1.0]
            sampling[axis] = bad
            assert code(sampling=sampling) == _ffi.CX_ERR_INVALID, (bad, axis)
    for radius2 in (-1.0, float("nan"), float("inf")):
        assert code(kind="mask", radius2=radius2) == _ffi.CX_ERR_INVALID
        ctx.distance_grid(0.5, "below", "float32", None, radius2, samples=A, download=True)      # (not read by the other kinds)
    assert code(side="signed", kind="mask", radius2=1.0) == _ffi.CX_ERR_INVALID
    _ffi.DIST_SIDES["inside"], _ffi.DIST_KINDS["float16"] = 3, 3
    try:
        assert code(side="inside") == _ffi.CX_ERR_INVALID
        assert code(kind="float16") == _ffi.CX_ERR_INVALID
    finally:
        del _ffi.DIST_SIDES["inside"], _ffi.DIST_KINDS["float16"]
    t = torch.from_numpy(A).cuda()
    torch.cuda.synchronize()
    dev = (t.data_ptr(), t.dtype, A.shape)
    call = ctx.lib.cx_grid_distance3d
    for dtype in (7, -1):
        assert call(ctx.handle, t.data_ptr(), dtype, 1, 4, 5, 6, 0.5, None, 0, 1, 0.0, None, None, None) == _ffi.CX_ERR_INVALID
    for shape in ((0, 5, 6), (4, -1, 6), (1 << 15, 1 << 15, 1)):      # an empty axis, and more than 2^29 samples
        assert call(ctx.handle, t.data_ptr(), 0, 1, shape[0], shape[1], shape[2], 0.5, None, 0, 1, 0.0, None, None, None) == _ffi.CX_ERR_INVALID
    assert call(None, t.data_ptr(), 0, 1, 4, 5, 6, 0.5, None, 0, 1, 0.0, None, None, None) == _ffi.CX_ERR_INVALID
    # an output that overlaps the input: the same memory, its last sample, the sample in front of it
    assert code(samples=dev, out=t.data_ptr()) == _ffi.CX_ERR_INVALID
    assert code(samples=dev, out=t.data_ptr() + 4 * (A.size - 1)) == _ffi.CX_ERR_INVALID
    assert code(samples=dev, kind="mask", out=t.data_ptr() + 4 * A.size - 1) == _ffi.CX_ERR_INVALID
    big = torch.zeros(3 * A.size, dtype=torch.float32, device="cuda")
    inner = big[A.size:2 * A.size]
    inner.copy_(t.reshape(-1))
    torch.cuda.synchronize()
    assert code(samples=(inner.data_ptr(), inner.dtype, A.shape), out=big.data_ptr() + 4) == _ffi.CX_ERR_INVALID
    assert code(samples=(inner.data_ptr(), inner.dtype, A.shape), kind="squared", out=big.data_ptr() + 8 * A.size - 8) == _ffi.CX_ERR_INVALID
    # next to it is fine
    ctx.distance_grid(0.5, "signed", samples=(inner.data_ptr(), inner.dtype, A.shape), out=big.data_ptr())
    same(big[:A.size].cpu().numpy().reshape(A.shape), R.distance(A, 0.5, "signed"))


def test_a_pointer_into_the_pending_result():
    "planes 1 to 5 of a pending uint8 mask as the samples of the next call, whose result the context keeps again"
    from contourist_amd import _ffi
    A = uniform((6, 9, 70), 41)
    first = R.mask(A, 0.97, "below", 2.0)
    assert 0 < first[1:].sum() < first[1:].size
    c = _ffi.Context()
    try:
        _, ptr = c.distance_grid(0.97, "below", "mask", radius2=2.0, samples=A)
        n_sites, got = c.distance_grid(0.5, "below", "float32", samples=(ptr + 9 * 70, "uint8", (5, 9, 70)), download=True)
        assert n_sites == int(first[1:].sum())
        same(got, R.distance(first[1:], 0.5, "below"))
        assert c.distance_result()[::2] == ((5, 9, 70), "float32")
    finally:
        c.close()
