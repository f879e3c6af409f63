"""cx_grid_reconstruct3d (csrc/cx_recon.hip) against its numpy restatement (tests/recon_ref.py), byte for byte: shapes around the kernel's
tile, values that have to travel through many tiles and back into tiles that had settled, every sample type from the host and from a
device tensor, the four marker kinds, contourist_amd.volume against scipy, the routes with no host copy, what a call leaves alone and
what a bind resets, the error codes, and twice the same bytes."""
import itertools

import numpy as np
import pytest

import rank_ref as R
import recon_ref as C

pytestmark = pytest.mark.gpu

# a workgroup owns 8 x 8 x 64 samples (CXR_T0 x CXR_T1 x CXR_T2), the lanes of a wave along the last axis
TILE = (8, 8, 64)
SHAPES = [(TILE[0] + 1, TILE[1] + 2, 1), (TILE[0] + 2, TILE[1] + 1, TILE[2] - 1), (TILE[0] + 1, TILE[1] + 3, TILE[2]),
          (TILE[0] + 3, TILE[1] + 1, TILE[2] + 1), (TILE[0] + 1, TILE[1] + 2, 2 * TILE[2] + 3)]
SMALL_SHAPES = [(1, 1, 5), (2, 2, 2), (3, 1, 70)]
TORCH_NAMES = {"float32": "float32", "uint8": "uint8", "int8": "int8", "uint16": "int16", "int16": "int16", "float16": "float16", "bfloat16": "bfloat16"}
CONNECTIVITIES = (1, 2, 3)


def round_cap(shape):
    "the bound of the host's loop over the rounds: a path without repeats has fewer steps than the array has samples"
    return int(np.prod(shape)) + 8


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def typed(name, shape, seed, levels=5):
    """few distinct values of the type (ties everywhere), the ends of an integer type among them -> (the mask as numpy: uint16 bit patterns
    for bfloat16; a marker = the mask minus random amounts with some samples above it; the dtype argument of the restatement)"""
    rng = np.random.RandomState(seed)
    steps = rng.randint(0, levels, size=shape)
    down = rng.randint(0, 4, size=shape) * (rng.uniform(size=shape) < 0.8)
    marks = np.where(rng.uniform(size=shape) < 0.08, steps + 2, steps - down)
    if name in R.FLOATS:
        a, g = (steps * 0.25 - 0.5).astype(np.float32), (marks * 0.25 - 0.5).astype(np.float32)
        if name == "float16":
            return a.astype(np.float16), g.astype(np.float16), None
        if name == "bfloat16":      # (multiples of 0.25 of this size are bfloat16 values)
            return (a.view(np.uint32) >> 16).astype(np.uint16), (g.view(np.uint32) >> 16).astype(np.uint16), "bfloat16"
        return a, g, None
    info = np.iinfo(np.dtype(name))
    a, g = steps + info.min, np.clip(marks + info.min, info.min, info.max)
    top = rng.uniform(size=shape) < 0.1      # the upper end of the type too
    a, g = np.where(top, info.max, a), np.where(top, info.max - down, g)
    return a.astype(name), g.astype(name), None


def on_device(name, a):
    "a numpy array (uint16 bit patterns for bfloat16) as a device tensor of the type"
    import torch
    if name == "bfloat16":
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a.view(np.int16) if name == "uint16" else a).cuda()


def run(ctx, A, marker, dtype=None, samples=None, marker_arg=None, **kw):
    "both kinds of output of one reconstruction == the restatement, byte for byte, with its counts -> the stats of the last call"
    for out_kind in ("values", "changed"):
        want, n_changed, n_clamped = C.reconstruct(A, marker, out_kind=out_kind, dtype=dtype, **kw)
        stats, got = ctx.reconstruct_grid(marker if marker_arg is None else marker_arg, out_kind=out_kind, samples=A if samples is None else samples, download=True, **kw)
        assert R.same_bytes(got, want), (A.shape, out_kind, kw)
        assert (stats["n_changed"], stats["n_clamped"]) == (n_changed, n_clamped), (A.shape, out_kind, kw, stats)
        assert 1 <= stats["rounds"] <= round_cap(A.shape) and stats["tile_visits"] >= stats["rounds"]
    return stats


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("method", C.METHODS)
def test_shapes_around_the_tile(ctx, method, connectivity):
    clamped = 0
    for n, shape in enumerate(SHAPES + SMALL_SHAPES):
        A, G, _ = typed("uint8", shape, 10 + n)
        clamped += run(ctx, A, G, method=method, connectivity=connectivity)["n_clamped"]
    assert clamped > 0


def corridor_along_axis2(shape):
    "a corridor one sample wide in the plane i = 1: along axis 2 in every second row, turning at alternating ends -> (mask, its cells in order)"
    cells = []
    for n, j in enumerate(range(0, shape[1], 2)):
        ks = list(range(shape[2])) if n % 2 == 0 else list(range(shape[2] - 1, -1, -1))
        cells += [(1, j, k) for k in ks]
        if j + 2 < shape[1]:
            cells.append((1, j + 1, ks[-1]))
    return cells


def filled(shape, cells, value=200):
    A = np.zeros(shape, dtype=np.uint8)
    A[tuple(np.array(cells).T)] = value
    return A


def seed_of(shape, cell, value=200):
    G = np.zeros(shape, dtype=np.uint8)
    G[cell] = value
    return G


@pytest.mark.parametrize("plane", ["along axis 2", "in the (0, 1) plane"])
def test_a_value_travels_a_corridor_through_many_tiles(ctx, plane):
    if plane == "along axis 2":
        shape = (3, 2 * TILE[1] + 1, 2 * TILE[2] + 2)
        cells = corridor_along_axis2(shape)
    else:      # the same corridor with the axes turned: rows along axis 1 in the plane k = 1
        shape = (2 * TILE[0] + 1, 2 * TILE[1] + 2, 3)
        cells = [(j, k, i) for i, j, k in corridor_along_axis2((3, shape[0], shape[1]))]
    A = filled(shape, cells)
    assert len(set(cells)) == len(cells) and int((A == 200).sum()) == len(cells)
    for end in (cells[0], cells[-1]):
        G = seed_of(shape, end)
        stats, got = ctx.reconstruct_grid(G, samples=A, download=True)
        # the whole corridor fills: the result is the mask itself, so no sample differs from it, and everything else stays zero
        assert R.same_bytes(got, A) and stats["n_changed"] == 0 and int((got == 0).sum()) == A.size - len(cells)
        assert 1 <= stats["rounds"] <= round_cap(shape)
        assert R.same_bytes(got, C.reconstruct(A, G)[0])
        # one sample of the corridor closed: it fills up to there, the rest differs from the mask
        B = A.copy()
        B[cells[len(cells) // 2]] = 0
        stats, got = ctx.reconstruct_grid(G, samples=B, download=True)
        want, n_changed, _ = C.reconstruct(B, G)
        assert R.same_bytes(got, want) and stats["n_changed"] == n_changed and 0 < n_changed < len(cells)


@pytest.mark.parametrize("needs", [2, 3])
def test_diagonal_staircases(ctx, needs):
    "every step differs on `needs` axes, and the step in the middle leaves the tile over its edge (2) or its corner (3)"
    if needs == 2:
        shape = (3, 2 * TILE[1] + 1, 2 * TILE[2] + 2)
        cells = [(1, d, TILE[2] - TILE[1] + d) for d in range(2 * TILE[1] + 1)]
    else:
        shape = (2 * TILE[0] + 1, 2 * TILE[1] + 1, 2 * TILE[2] + 2)
        cells = [(d, d, TILE[2] - TILE[1] + d) for d in range(2 * TILE[1] + 1)]
    assert (TILE[0] - 1 if needs == 3 else 1, TILE[1] - 1, TILE[2] - 1) in cells
    A = filled(shape, cells)
    for end, connectivity in itertools.product((cells[0], cells[-1]), CONNECTIVITIES):
        G = seed_of(shape, end)
        stats, got = ctx.reconstruct_grid(G, connectivity=connectivity, samples=A, download=True)
        want, n_changed, _ = C.reconstruct(A, G, connectivity=connectivity)
        assert R.same_bytes(got, want) and stats["n_changed"] == n_changed
        assert R.same_bytes(got, A if connectivity >= needs else G)


def test_a_tile_that_settled_is_opened_again(ctx):
    shape = (3, 3, 3 * TILE[2] + 8)
    A = np.full(shape, 200, dtype=np.uint8)
    G = np.zeros(shape, dtype=np.uint8)
    G[-1, -1, -1], G[0, 0, 0] = 100, 200
    for connectivity in CONNECTIVITIES:
        stats, got = ctx.reconstruct_grid(G, connectivity=connectivity, samples=A, download=True)
        assert R.same_bytes(got, A) and stats["n_changed"] == 0 and stats["rounds"] >= 2
    stats, got = ctx.reconstruct_grid(255 - G, method="erosion", samples=255 - A, download=True)
    assert R.same_bytes(got, 255 - A)


@pytest.mark.parametrize("name", R.TYPES)
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    shape = (9, 10, 70)
    A, G, dtype = typed(name, shape, 9)
    ta, tg = on_device(name, A), on_device(name, G)
    torch.cuda.synchronize()
    host = ((A, "bfloat16", shape), (G, "bfloat16", shape)) if dtype else (A, G)
    dev = ((ta.data_ptr(), name, shape), (tg.data_ptr(), name, shape))
    for method, connectivity in itertools.product(C.METHODS, (1, 3)):
        for samples, marker_arg in (host, dev):
            run(ctx, A, G, dtype=dtype, samples=samples, marker_arg=marker_arg, method=method, connectivity=connectivity)
            for kind in ("step", "rim"):
                run(ctx, A, kind, dtype=dtype, samples=samples, method=method, connectivity=connectivity, faces=9)


def test_misaligned_device_slice_callers_output_and_host_copy(ctx):
    import torch
    from contourist_amd import _ffi
    shape = (5, 9, 67)
    n = int(np.prod(shape))
    for name in R.TYPES:
        flat, gflat, dtype = typed(name, (n + 1,), 30)
        ta, tg = on_device(name, flat)[1:], on_device(name, gflat)[1:]      # the input pointers are one element off their allocations
        assert ta.data_ptr() % 16 != 0
        A, G = flat[1:].reshape(shape), gflat[1:].reshape(shape)
        for out_kind in ("values", "changed"):
            want, n_changed, n_clamped = C.reconstruct(A, G, connectivity=2, out_kind=out_kind, dtype=dtype)
            out = torch.full((n + 2,), 7, dtype=getattr(torch, TORCH_NAMES[name]) if out_kind == "values" else torch.uint8, device="cuda")
            guard = out[:1].cpu().view(torch.uint8).numpy().tobytes()      # the bytes of one element of the fill
            torch.cuda.synchronize()
            host_out = np.empty(shape, dtype=want.dtype)
            st = np.zeros(4, dtype=np.int64)
            rc = ctx.lib.cx_grid_reconstruct3d(ctx.handle, ta.data_ptr(), _ffi.DTYPE_CODES[name], 1, shape[0], shape[1], shape[2], tg.data_ptr(),
                                               _ffi.RECON_MARKERS["array"], 0.0, 0, _ffi.RECON_METHODS["dilation"], 2, _ffi.RECON_OUTS[out_kind],
                                               out[1:].data_ptr(), host_out.ctypes.data, st.ctypes.data)
            torch.cuda.synchronize()
            assert rc == _ffi.CX_OK and (int(st[0]), int(st[1])) == (n_changed, n_clamped)
            raw, size = out.cpu().view(torch.uint8).numpy().tobytes(), want.dtype.itemsize
            assert len(guard) == size and raw[:size] == guard and raw[-size:] == guard      # nothing written around the result
            assert raw[size:-size] == want.tobytes() and host_out.tobytes() == want.tobytes(), (name, out_kind)
            with pytest.raises(_ffi.CxError) as e:      # with an output of the caller's the context holds no result
                ctx.reconstruct_result()
            assert e.value.code == _ffi.CX_ERR_STATE


def test_shift_saturates_and_rounds_once(ctx):
    rng = np.random.RandomState(4)
    shape = (9, 10, 70)
    for name in ("uint8", "int8", "int16", "uint16"):
        A, _, _ = typed(name, shape, 40)      # holds both ends of the type
        info = np.iinfo(A.dtype)
        assert A.min() == info.min and A.max() == info.max
        for h, method in itertools.product((1, 3, 300, 1e9), C.METHODS):
            run(ctx, A, "shift", h=h, method=method)
    # the sum is computed in float64 and rounded to the type once: h is no value of the type, the samples spread over many binades
    base = (rng.standard_normal(shape) * np.exp2(rng.randint(-12, 12, size=shape))).astype(np.float32)
    base[rng.uniform(size=shape) < 0.02] = np.inf
    base[rng.uniform(size=shape) < 0.02] = -np.inf
    base[rng.uniform(size=shape) < 0.02] = np.nan
    for name, A, dtype in (("float32", base, None), ("float16", base.astype(np.float16), None), ("bfloat16", C.round_bfloat16(base.astype(np.float64)), "bfloat16")):
        samples = (A, "bfloat16", shape) if dtype else A
        for h, method in itertools.product((0.1, 1.0 + 2.0 ** -12, 3.0e-5, 1.0e6), C.METHODS):
            run(ctx, A, "shift", dtype=dtype, samples=samples, h=h, method=method, connectivity=2)


@pytest.mark.parametrize("name", R.TYPES)
def test_step_gives_the_regional_extrema(ctx, name):
    shape = (9, 10, 70)
    A, _, dtype = typed(name, shape, 50, levels=3)
    samples = (A, "bfloat16", shape) if dtype else A
    for method, connectivity in itertools.product(C.METHODS, CONNECTIVITIES):
        stats = run(ctx, A, "step", dtype=dtype, samples=samples, method=method, connectivity=connectivity)
        assert 0 < stats["n_changed"] < A.size
    rim = C.reconstruct(A, "step", out_kind="changed", dtype=dtype)[0]
    assert rim[0].any() and rim[:, :, -1].any()      # plateaus that touch the rim are among them


def test_step_special_cases(ctx):
    # -0.0 beside +0.0 are two values; NaN is the top, the infinities are the ends
    Z = np.array([0.0, -0.0, -0.0, 0.0, np.inf, np.nan, -np.inf, 1.0, -np.inf, -np.inf], dtype=np.float32).reshape(1, 2, 5)
    for A, dtype in ((Z, None), (Z.astype(np.float16), None), (C.round_bfloat16(Z.astype(np.float64)), "bfloat16")):
        for method, connectivity in itertools.product(C.METHODS, (1, 2)):
            run(ctx, A, "step", dtype=dtype, samples=(A, "bfloat16", A.shape) if dtype else A, method=method, connectivity=connectivity)
    got = ctx.reconstruct_grid("step", out_kind="changed", samples=np.ascontiguousarray(Z[:, :1, :4]), download=True)[1]
    assert got.reshape(-1).tolist() == [1, 0, 0, 1]
    # an integer array that is the extreme of its type everywhere has no predecessor: one regional extremum, all ones
    for A, method in ((np.zeros((3, 9, 70), np.uint8), "dilation"), (np.full((3, 9, 70), -128, np.int8), "dilation"), (np.full((3, 9, 70), 255, np.uint8), "erosion"),
                      (np.full((2, 2, 2), 32767, np.int16), "erosion"), (np.full((3, 9, 70), 7, np.uint8), "dilation"), (np.full((3, 9, 70), 255, np.uint8), "dilation")):
        stats = run(ctx, A, "step", method=method)
        got = ctx.reconstruct_grid("step", method=method, out_kind="changed", samples=A, download=True)[1]
        assert got.all()


def test_rim_every_face_and_all_six(ctx):
    for shape, seed in (((9, 10, 70), 60), ((1, 9, 70), 61), ((9, 1, 3), 62)):
        A, _, _ = typed("int16", shape, seed)
        for faces, method in itertools.product([1, 2, 4, 8, 16, 32, 63, 5, 40], C.METHODS):
            run(ctx, A, "rim", faces=faces, method=method, connectivity=1 + faces % 3)


def test_volume_module_against_scipy_and_the_restatement():
    import scipy.ndimage as ndi
    import torch
    from contourist_amd import volume
    rng = np.random.RandomState(3)
    shape = (9, 13, 70)
    mask = rng.uniform(size=shape) < 0.4
    seeds = mask & (rng.uniform(size=shape) < 0.03)
    blobs = ndi.binary_dilation(rng.uniform(size=shape) < 0.05, ndi.generate_binary_structure(3, 1))
    blobs[2:7, 3:8, 4:9] = True
    blobs[3:6, 4:7, 5:8] = False

    def both(call, args, want):
        got = call(*args)
        got_t = call(*[torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in args])
        assert isinstance(got, np.ndarray) and R.same_bytes(got, want)
        assert got_t.is_cuda and got_t.shape == torch.Size(want.shape) and R.same_bytes(got_t.cpu().numpy(), want)

    for c in CONNECTIVITIES:
        st = ndi.generate_binary_structure(3, c)
        want = ndi.binary_propagation(seeds, st, mask=mask).astype(np.uint8)
        both(lambda s, m: volume.propagate(s, m, c), (seeds, mask), want)
        both(lambda s, m: volume.propagate(s, m, c), (seeds.astype(np.uint8) * 7, mask.astype(np.uint8) * 3), want)
        both(lambda s: volume.fill_holes_grey(s, c), (blobs,), ndi.binary_fill_holes(blobs, st).astype(np.uint8))
    assert ndi.binary_fill_holes(blobs).sum() > blobs.sum()
    for A in ((rng.randint(-4, 5, size=shape) * 0.25).astype(np.float32), rng.randint(0, 7, size=shape).astype(np.uint8), rng.randint(-3, 4, size=shape).astype(np.int16)):
        G = (A - rng.randint(0, 3, size=shape) * (1 if A.dtype.kind != "f" else 0.25)).clip(A.min(), None).astype(A.dtype)
        h = 2 if A.dtype.kind != "f" else 0.6
        both(lambda g, f: volume.reconstruct(g, f), (G, A), C.reconstruct(A, G)[0])
        both(lambda g, f: volume.reconstruct(g, f, "erosion", 2), (A, G), C.reconstruct(G, A, method="erosion", connectivity=2)[0])
        both(lambda s: volume.h_maxima(s, h), (A,), C.reconstruct(A, "shift", h=h)[0])
        both(lambda s: volume.h_minima(s, h, 3), (A,), C.reconstruct(A, "shift", h=h, method="erosion", connectivity=3)[0])
        both(lambda s: volume.h_domes(s, h), (A,), C.reconstruct(A, "shift", h=h, out_kind="changed")[0])
        both(lambda s: volume.h_basins(s, h), (A,), C.reconstruct(A, "shift", h=h, method="erosion", out_kind="changed")[0])
        both(lambda s: volume.regional_maxima(s, 2), (A,), C.reconstruct(A, "step", connectivity=2, out_kind="changed")[0])
        both(lambda s: volume.regional_minima(s), (A,), C.reconstruct(A, "step", method="erosion", out_kind="changed")[0])
        both(lambda s: volume.fill_holes_grey(s), (A,), C.reconstruct(A, "rim", method="erosion")[0])
        both(lambda s: volume.clear_border_grey(s), (A,), C.reconstruct(A, "rim")[0])
        both(lambda s: volume.clear_border_grey(s, faces=3, connectivity=2, mask=True), (A,), C.reconstruct(A, "rim", faces=3, connectivity=2, out_kind="changed")[0])
    # float64 goes through float32; two dimensions and one: the missing leading axes have no faces
    D = rng.randint(-4, 5, size=(23, 70)) * 0.25
    want = C.reconstruct(R.pad3(D.astype(np.float32)), "rim", faces=0b111100)[0].reshape(D.shape)
    both(lambda s: volume.clear_border_grey(s), (D,), want)
    assert (want != D).any()
    want = C.reconstruct(R.pad3(D[3].astype(np.float32)), "rim", faces=0b110000, method="erosion")[0].reshape(-1)
    both(lambda s: volume.fill_holes_grey(s), (D[3],), want)
    assert (want != D[3]).any()
    both(lambda s: volume.clear_border_grey(s, faces=2), (D[3],), C.reconstruct(R.pad3(D[3].astype(np.float32)), "rim", faces=0b100000)[0].reshape(-1))
    both(lambda s: volume.regional_maxima(s), (D[3],), C.reconstruct(R.pad3(D[3].astype(np.float32)), "step", out_kind="changed")[0].reshape(-1))


def test_distance_then_regional_maxima_then_labels_without_a_host_copy():
    import distance_ref
    import label_ref
    from contourist_amd import _ffi
    rng = np.random.RandomState(5)
    A = (rng.standard_normal((9, 10, 70)) * 3.0).astype(np.float32)
    D = distance_ref.distance(A, 1.5, "below")
    M = C.reconstruct(D, "step", connectivity=3, out_kind="changed")[0]
    labels, k = label_ref.label(M, 0.5, "high", 3)
    assert k > 3
    c = _ffi.Context()
    try:
        _, dptr = c.distance_grid(1.5, "below", "float32", samples=A)
        stats, mptr = c.reconstruct_grid("step", connectivity=3, out_kind="changed", samples=(dptr, "float32", A.shape))
        assert c.reconstruct_result() == (A.shape, mptr, "uint8", "changed") and c.distance_result()[1] == dptr and stats["n_changed"] == int(M.sum())
        got_k, got = c.label_grid(0.5, "high", 3, samples=(mptr, "uint8", A.shape), download=True)
        assert got_k == k and np.array_equal(got, labels)
        # the pending mask is a legal input of the distance transform, the rank filters and the reconstruction itself
        n_sites, dist = c.distance_grid(0.5, "below", "float32", samples=(mptr, "uint8", A.shape), download=True)
        assert n_sites == int(M.sum()) and dist.tobytes() == distance_ref.distance(M, 0.5, "below").tobytes()
        assert R.same_bytes(c.rank_grid(3, 26, samples=(mptr, "uint8", A.shape), download=True)[1], R.rank_filter(M, 26, 3))
        again = c.reconstruct_grid("rim", method="erosion", samples=(mptr, "uint8", A.shape), download=True)[1]
        assert R.same_bytes(again, C.reconstruct(M, "rim", method="erosion")[0])
        # the result of a call as the mask of the next one
        _, vptr = c.reconstruct_grid("rim", method="erosion", samples=M)
        twice = c.reconstruct_grid("shift", h=1, samples=(vptr, "uint8", A.shape), download=True)[1]
        assert R.same_bytes(twice, C.reconstruct(C.reconstruct(M, "rim", method="erosion")[0], "shift", h=1)[0])
    finally:
        c.close()


def _mesh(c, value):
    from contourist_amd import _ffi
    counts = c.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    return counts, c.download_level0_records(counts)


def _same_mesh(a, b):
    (c0, m0), (c1, m1) = a, b
    return c0 == c1 and np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1].view(np.uint32), m1[1].view(np.uint32)) and np.array_equal(m0[2], m1[2])


def test_reconstruct_bind_march_and_what_a_call_leaves_alone():
    from contourist_amd import _ffi
    rng = np.random.RandomState(19)
    A = (rng.standard_normal((12, 13, 70)) * 3.0).astype(np.float32)
    want = C.reconstruct(A, "shift", h=2.5, connectivity=2)[0]
    assert not np.array_equal(want, A)
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c, fresh = _ffi.Context(), _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)                                                # the other five pending results
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        c.resample_grid(np.diag([1.0, 0.5, 1.0]), np.zeros(3), A.shape)
        res = c.resample_result()
        _, qptr = c.rank_grid(3, 13)
        stats, rptr = c.reconstruct_grid("shift", h=2.5, connectivity=2)          # of the bound grid, into the context
        c.reconstruct_grid("step", samples=typed("uint8", (5, 6, 7), 1)[0], download=True)      # of other samples
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts               # the grid is the one uploaded
        assert (c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k) and c.resample_result() == res
                and c.rank_result() == (A.shape, qptr, "float32"))
        stats, rptr = c.reconstruct_grid("shift", h=2.5, connectivity=2)
        assert c.reconstruct_result() == (A.shape, rptr, "float32", "values") and stats["n_changed"] == int((want != A).sum())
        # bind: as after an upload; the other five results stay
        c.bind_reconstructed()
        for gone in (c.counts, lambda: c.download_level1(p), c.reconstruct_result, c.bind_reconstructed):
            with pytest.raises(_ffi.CxError) as e:
                gone()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert (c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k) and c.resample_result() == res
                and c.rank_result() == (A.shape, qptr, "float32"))
        assert c.shape == A.shape and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        fresh.upload_grid(want)
        got, ref = _mesh(c, 0.1), _mesh(fresh, 0.1)
        assert _same_mesh(got, ref) and got[0]["n_triangles"] > 1000
        # a CHANGED mask binds as uint8
        c.reconstruct_grid("step", out_kind="changed")
        c.bind_reconstructed()
        assert c.grid_info() == dict(dtype="uint8", device_bytes=A.size)
        # a result with an axis of length 1 is refused and stays pending
        _, rptr = c.reconstruct_grid("step", samples=A[:1])
        with pytest.raises(_ffi.CxError) as e:
            c.bind_reconstructed()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.reconstruct_result() == ((1, 13, 70), rptr, "float32", "values") and c.shape == A.shape
    finally:
        c.close()
        fresh.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import torch
    from contourist_amd import _ffi
    A, G, _ = typed("uint8", (4, 5, 6), 21)
    F = A.astype(np.float32)

    def code(marker="step", samples=A, **kw):
        with pytest.raises(_ffi.CxError) as e:
            ctx.reconstruct_grid(marker, samples=samples, **kw)
        return e.value.code

    fresh = _ffi.Context()
    try:
        for call in (lambda: fresh.reconstruct_grid("step"), fresh.reconstruct_result, fresh.bind_reconstructed):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert fresh.lib.cx_grid_reconstruct3d(fresh.handle, None, 0, 1, 0, 0, 0, None, 2, 0.0, 0, 0, 1, 0, None, None, None) == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    t, tg = torch.from_numpy(A).cuda(), torch.from_numpy(G).cuda()
    torch.cuda.synchronize()
    call = ctx.lib.cx_grid_reconstruct3d

    def raw(mask=None, dtype=1, shape=(4, 5, 6), marker=None, kind=2, h=0.0, faces=0, method=0, connectivity=1, out_kind=0, out=None, handle=None):
        return call(ctx.handle if handle is None else handle, t.data_ptr() if mask is None else mask, dtype, 1, shape[0], shape[1], shape[2], marker, kind, h, faces,
                    method, connectivity, out_kind, out, None, None)

    assert raw() == _ffi.CX_OK and raw(kind=0, marker=tg.data_ptr()) == _ffi.CX_OK and raw(kind=3, faces=63) == _ffi.CX_OK and raw(kind=1, h=2.0) == _ffi.CX_OK
    for bad in (dict(method=2), dict(method=-1), dict(kind=4), dict(kind=-1), dict(out_kind=2), dict(out_kind=-1), dict(connectivity=0), dict(connectivity=4),
                dict(dtype=7), dict(dtype=-1), dict(kind=3, faces=0), dict(kind=3, faces=64), dict(kind=3, faces=-1), dict(kind=0, marker=None),
                dict(kind=1, h=0.0), dict(kind=1, h=-1.0), dict(kind=1, h=float("nan")), dict(kind=1, h=float("inf")), dict(kind=1, h=1.5),
                dict(shape=(0, 5, 6)), dict(shape=(4, -1, 6))):
        assert raw(**bad) == _ffi.CX_ERR_INVALID, bad
    assert call(None, t.data_ptr(), 1, 1, 4, 5, 6, None, 2, 0.0, 0, 0, 1, 0, None, None, None) == _ffi.CX_ERR_INVALID
    for shape in ((1 << 16, 1 << 16, 1), (1 << 11, 1 << 11, (1 << 9) + 1), (1 << 32, 1, 1)):      # more than 2^31 samples
        assert raw(shape=shape) == _ffi.CX_ERR_UNSUPPORTED
    ctx.reconstruct_grid("shift", h=1.5, samples=F)      # a fraction is a legal h of a float type
    assert code("shift", h=1.5) == _ffi.CX_ERR_INVALID and code(None) == _ffi.CX_ERR_INVALID
    # an output that overlaps the mask or the marker: the same memory, its last sample, the sample in front of it
    big = torch.zeros(5 * A.size, dtype=torch.uint8, device="cuda")
    m_in, g_in = big[A.size:2 * A.size], big[3 * A.size:4 * A.size]
    m_in.copy_(t.reshape(-1))
    g_in.copy_(tg.reshape(-1))
    torch.cuda.synchronize()
    src, mark = (m_in.data_ptr(), "uint8", A.shape), (g_in.data_ptr(), "uint8", A.shape)
    for inner in (m_in, g_in):
        for out in (inner.data_ptr(), inner.data_ptr() + A.size - 1, inner.data_ptr() - A.size + 1):
            assert code(mark, samples=src, out=out) == _ffi.CX_ERR_INVALID
    assert code("step", samples=src, out=m_in.data_ptr()) == _ffi.CX_ERR_INVALID
    ctx.reconstruct_grid("step", samples=src, out=g_in.data_ptr())      # (no marker array: that memory is free)
    g_in.copy_(tg.reshape(-1))
    torch.cuda.synchronize()
    # next to them is fine
    ctx.reconstruct_grid(mark, samples=src, out=big[2 * A.size:].data_ptr())
    ctx.synchronize()
    assert big[2 * A.size:3 * A.size].cpu().numpy().reshape(A.shape).tobytes() == C.reconstruct(A, G)[0].tobytes()


def test_twice_the_same_bytes_and_counts(ctx):
    "2^18 samples, 64 tiles: the tiles of a launch race, the result does not"
    A, G, _ = typed("float32", (16, 64, 256), 12, levels=9)
    for marker, kw in ((G, dict(connectivity=3)), ("shift", dict(h=0.6)), ("step", dict(method="erosion", connectivity=2)), ("rim", dict(faces=33))):
        want, n_changed, n_clamped = C.reconstruct(A, marker, **kw)
        stats, got = ctx.reconstruct_grid(marker, samples=A, download=True, **kw)
        ctx.reconstruct_grid("step", samples=typed("uint8", (3, 3, 3), 1)[0], download=True)      # (the scratch is reused in between)
        stats2, again = ctx.reconstruct_grid(marker, samples=A, download=True, **kw)
        assert R.same_bytes(got, want) and again.tobytes() == got.tobytes()
        assert (stats["n_changed"], stats["n_clamped"]) == (n_changed, n_clamped) == (stats2["n_changed"], stats2["n_clamped"])


def test_a_pointer_into_the_pending_result():
    "planes 1 to 5 of the pending result as the mask of the next call, whose result the context keeps again"
    from contourist_amd import _ffi
    A, G, _ = typed("uint8", (6, 9, 70), 41)
    first = C.reconstruct(A, G)[0]
    want, n_changed, n_clamped = C.reconstruct(np.ascontiguousarray(first[1:]), "step")
    assert n_changed > 0
    c = _ffi.Context()
    try:
        _, ptr = c.reconstruct_grid(G, samples=A)
        stats, got = c.reconstruct_grid("step", samples=(ptr + 9 * 70, "uint8", (5, 9, 70)), download=True)
        assert (stats["n_changed"], stats["n_clamped"]) == (n_changed, n_clamped) and R.same_bytes(got, want)
        assert c.reconstruct_result()[::2] == ((5, 9, 70), "uint8")
    finally:
        c.close()
