"""cx_grid_rank3d (csrc/cx_rank.hip) against its numpy restatement (tests/rank_ref.py), byte for byte: shapes around the kernels' tile,
the sizes, footprints, ranks, origins and boundary rules that reach the general kernel and the separable minimum / maximum, every
sample type from the host and from a device tensor, misaligned device slices, a caller's output, the special values of the floats,
contourist_amd.volume against scipy, the end-to-end routes with no host copy, what a call leaves alone and what a bind resets, the
error codes."""
import itertools
import os

import numpy as np
import pytest

import rank_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# a workgroup of either kernel owns 4 x 4 x 64 outputs (CXQ_T0 x CXQ_T1 x CXQ_T2), the lanes of a wave along the last axis
TILE = (4, 4, 64)
# the last axis 1, 63, 64, 65 and 131 long (a part of a tile, one tile less one, one, one and one sample, two and three samples); the
# other axes one tile and a partial one
SHAPES = [(TILE[0] + 1, TILE[1] + 2, 1), (TILE[0] + 2, TILE[1] + 1, TILE[2] - 1), (TILE[0] + 1, TILE[1] + 3, TILE[2]),
          (TILE[0] + 3, TILE[1] + 1, TILE[2] + 1), (TILE[0] + 1, TILE[1] + 2, 2 * TILE[2] + 3)]
# at size 7 the window is wider than the array on some axis, and a reflection wraps more than once
SMALL_SHAPES = [(1, 1, 5), (2, 2, 2), (3, 1, 70)]
BOXES = [(3, 3, 3), (1, 2, 5), (2, 3, 4), (7, 1, 3), (5, 5, 5), (7, 7, 7)]
TORCH_NAMES = {"float32": "float32", "uint8": "uint8", "int8": "int8", "uint16": "int16", "int16": "int16", "float16": "float16", "bfloat16": "bfloat16"}


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def field(shape, seed, dtype=np.float32):
    rng = np.random.RandomState(seed)
    if np.dtype(dtype).kind == "f":
        return (rng.standard_normal(shape) * 3.0).astype(dtype)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=shape).astype(dtype)


def random_mask(box, seed):
    rng = np.random.RandomState(seed)
    fp = rng.uniform(size=box) < 0.6
    fp.reshape(-1)[rng.randint(fp.size)] = True
    return fp


def ends_and_centre(box):
    return [tuple(0 for s in box), tuple(s // 2 for s in box), tuple(s - 1 for s in box)]


def ctypes_array(values):
    return np.asarray(values, dtype=np.int32)


def ranks_of(W):
    return sorted({0, 1 % W, W // 2, max(0, W - 2), W - 1})


def footprints():
    "name -> (box, footprint or None)"
    from contourist_amd import volume
    out = {}
    for box in BOXES:
        name = "%dx%dx%d" % box
        out[name + "-full"] = (box, None)
        out[name + "-mask"] = (box, random_mask(box, sum(box)))
    out["ball1"] = ((3, 3, 3), volume.ball(1))
    out["ball2"] = ((5, 5, 5), volume.ball(2))
    return out


FOOTPRINT_NAMES = ["%dx%dx%d-%s" % (b + (k,)) for b in BOXES for k in ("full", "mask")] + ["ball1", "ball2"]


def check_all(ctx, A, box, fp, dtype=None, samples=None):
    "every boundary rule (cval inside and outside the data's range), origin and rank: the device result == the restatement, byte for byte"
    name = R.type_name(A, dtype)
    inside, outside = (1.5, 64.0) if name in R.FLOATS else (3, 100)
    for (mode, cval), origin in itertools.product((("nearest", inside), ("reflect", outside), ("constant", inside), ("constant", outside)), ends_and_centre(box)):
        ordered = R.sorted_windows(A, box, fp, origin, mode, cval, dtype)
        for rank in ranks_of(len(ordered)):
            want = R.pick(ordered, rank, name)
            got = ctx.rank_grid(box, rank, fp, origin, mode, cval, samples=A if samples is None else samples, download=True)[1]
            assert R.same_bytes(got, want), (A.shape, box, fp is not None, mode, cval, origin, rank)


@pytest.mark.parametrize("name", FOOTPRINT_NAMES)
def test_sizes_footprints_ranks_origins_and_modes(ctx, name):
    "ranks 0 and W - 1 of a full box take the separable kernel, every other case the general one"
    box, fp = footprints()[name]
    for n, shape in enumerate(SHAPES):
        check_all(ctx, field(shape, 11 + n), box, fp)


@pytest.mark.parametrize("masked", [False, True])
def test_windows_wider_than_the_array(ctx, masked):
    box = (7, 7, 7)
    for n, shape in enumerate(SMALL_SHAPES):
        check_all(ctx, field(shape, 21 + n), box, random_mask(box, 5) if masked else None)


def test_separable_kernel_equals_the_general_one(ctx):
    "the minimum and maximum of a full box (no footprint: the separable kernel) and of an all-ones footprint (the general kernel)"
    for dtype, box in itertools.product((np.float32, np.int16, np.uint8), ((3, 3, 3), (2, 3, 4), (7, 7, 7), (1, 1, 1))):
        A = field(SHAPES[3], 31, dtype)
        W = int(np.prod(box))
        for rank, mode in itertools.product(sorted({0, W - 1}), R.MODES):
            a = ctx.rank_grid(box, rank, None, None, mode, 1, samples=A, download=True)[1]
            b = ctx.rank_grid(box, rank, np.ones(box, dtype=bool), None, mode, 1, samples=A, download=True)[1]
            assert R.same_bytes(a, b) and R.same_bytes(a, R.rank_filter(A, rank, box, None, None, mode, 1))


def test_many_tiles_and_twice_the_same_bytes(ctx):
    "2^18 outputs, 256 tiles: every XCD's run of the numbering"
    A = field((16, 64, 256), 12)
    A8 = field((16, 64, 256), 13, np.uint8)
    for S, box, fp, rank in ((A, (3, 3, 3), None, 13), (A, (3, 3, 3), None, 26), (A8, (5, 5, 5), None, 62), (A8, (3, 2, 3), random_mask((3, 2, 3), 1), 0)):
        want = R.rank_filter(S, rank, box, fp, None, "reflect")
        got = ctx.rank_grid(box, rank, fp, None, "reflect", samples=S, download=True)[1]
        ctx.rank_grid(3, 1, samples=field((3, 3, 3), 1), download=True)      # (the scratch is reused in between)
        again = ctx.rank_grid(box, rank, fp, None, "reflect", samples=S, download=True)[1]
        assert R.same_bytes(got, want) and again.tobytes() == got.tobytes()


def typed_field(name, shape, seed):
    "-> (the samples as numpy: uint16 bit patterns for bfloat16; the same as a device tensor; the dtype argument of the restatement)"
    import torch
    if name == "bfloat16":
        t = torch.from_numpy(field(shape, seed)).cuda().to(torch.bfloat16)
        return t.view(torch.int16).cpu().numpy().view(np.uint16), t, "bfloat16"
    A = field(shape, seed, np.dtype(name))
    if A.dtype.kind in "iu":      # the whole range, its ends included: the key's sign handling shows
        info = np.iinfo(A.dtype)
        A.reshape(-1)[:4] = [info.min, info.max, 0, info.min + 1 if info.min else 1]
    return A, torch.from_numpy(A.view(np.int16) if name == "uint16" else A).cuda(), None


@pytest.mark.parametrize("name", R.TYPES)
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    shape = (6, 7, 70)
    A, t, dtype = typed_field(name, shape, 9)
    torch.cuda.synchronize()
    host = (A, "bfloat16", shape) if dtype else A
    for box, fp in (((3, 2, 5), None), ((3, 2, 5), random_mask((3, 2, 5), 2))):
        check_all(ctx, A, box, fp, dtype=dtype, samples=host)
        check_all(ctx, A, box, fp, dtype=dtype, samples=(t.data_ptr(), name, shape))


def test_misaligned_device_slice_and_callers_output(ctx):
    import torch
    from contourist_amd import _ffi
    shape = (5, 9, 67)
    n = int(np.prod(shape))
    for name in R.TYPES:
        flat, flat_t, dtype = typed_field(name, (n + 1,), 30)
        t = flat_t[1:]      # the input pointer is one element off its allocation
        assert t.data_ptr() % 16 != 0
        A = flat[1:].reshape(shape)
        for box, fp, rank in (((3, 3, 3), None, 13), ((3, 3, 3), None, 0), ((2, 3, 4), random_mask((2, 3, 4), 4), 5)):
            want = R.rank_filter(A, rank, box, fp, None, "constant", 3, dtype)
            out = torch.full((n + 2,), 7, dtype=getattr(torch, TORCH_NAMES[name]), device="cuda")
            guard = out[:1].cpu().view(torch.uint8).numpy().tobytes()      # the bytes of one element of the fill
            torch.cuda.synchronize()
            got_shape, ptr = ctx.rank_grid(box, rank, fp, None, "constant", 3, samples=(t.data_ptr(), name, shape), out=out[1:].data_ptr())
            torch.cuda.synchronize()
            assert got_shape == shape and ptr == out[1:].data_ptr()
            raw, size = out.cpu().view(torch.uint8).numpy().tobytes(), want.dtype.itemsize
            assert len(guard) == size and raw[:size] == guard and raw[-size:] == guard      # nothing written around the result
            assert raw[size:-size] == want.tobytes(), (name, box, rank)
            with pytest.raises(_ffi.CxError) as e:      # with an output of the caller's the context holds no result
                ctx.rank_result()
            assert e.value.code == _ffi.CX_ERR_STATE


SPECIAL_F32 = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF]


@pytest.mark.parametrize("name", ["float32", "float16", "bfloat16"])
def test_float_special_values(ctx, name):
    """NaNs of both signs and with payloads, +-inf, -0.0 beside +0.0, denormals: a quarter of the samples, so that each is the selected
    element of some windows and an unselected element of others; the bit patterns equal the restatement's"""
    rng = np.random.RandomState(17)
    shape = (6, 7, 70)
    if name == "float32":
        special = np.array(SPECIAL_F32, dtype=np.uint32)
        A = field(shape, 14).view(np.uint32)
        dtype, U, qnan, inf = None, np.uint32, 0x7FC00000, 0x7F800000
    else:
        _, _, inf, qnan = R.FLOATS[name]
        low = (1 << (10 if name == "float16" else 7)) - 1      # the largest denormal
        special = np.array([qnan, qnan | 0x8000, inf + 1, 0x8000 | inf | 0x15, inf, inf | 0x8000, 0, 0x8000, 1, 0x8001, low, 0x8000 | low], dtype=np.uint16)
        base = field(shape, 14)
        A = base.astype(np.float16).view(np.uint16) if name == "float16" else (base.view(np.uint32) >> 16).astype(np.uint16)
        dtype, U = ("bfloat16" if name == "bfloat16" else None), np.uint16
    A = A.copy()
    at = rng.uniform(size=shape) < 0.25
    A[at] = special[rng.randint(len(special), size=int(at.sum()))]
    S = A if name == "bfloat16" else A.view(np.dtype(name))
    host = (S, "bfloat16", shape) if name == "bfloat16" else S
    mag = U((1 << (8 * A.dtype.itemsize - 1)) - 1)
    seen = set()
    for box, fp in (((3, 3, 3), None), ((2, 1, 3), None), ((3, 3, 3), random_mask((3, 3, 3), 6))):
        for mode in R.MODES:
            ordered = R.sorted_windows(S, box, fp, None, mode, 0.5, dtype)
            W = len(ordered)
            has_nan = ordered[W - 1] == U(~U(0))
            for rank in ranks_of(W):
                want = R.pick(ordered, rank, name)
                got = ctx.rank_grid(box, rank, fp, None, mode, 0.5, samples=host, download=True)[1]
                assert R.same_bytes(got, want), (box, mode, rank)
                bits = got.view(U)
                nan_out = (bits & mag) > U(inf)
                assert np.all(bits[nan_out] == U(qnan))                      # a selected NaN is the canonical one
                if (has_nan & ~nan_out).any():
                    seen.add("nan in the window, not selected")
                seen.update(int(b) for b in np.unique(bits[np.isin(bits, special)]))
    assert "nan in the window, not selected" in seen
    assert seen >= {int(b) for b in special if (int(b) & int(mag)) <= inf} | {qnan}, "each special value is selected somewhere"


def test_volume_module_against_scipy():
    import scipy.ndimage as ndi
    import torch
    from contourist_amd import volume
    rng = np.random.RandomState(3)
    for A in ((rng.randint(-4, 5, size=(9, 13, 70)) * 0.25).astype(np.float32), rng.randint(0, 7, size=(9, 13, 70)).astype(np.uint8),
              rng.randint(-3, 4, size=(9, 13, 70)).astype(np.int16), (rng.randint(-4, 5, size=(9, 13, 70)) * 0.25).astype(np.float64)):
        t = torch.from_numpy(A).cuda()
        out_dtype = np.float32 if A.dtype == np.float64 else A.dtype      # types the kernels do not read are converted to float32 first

        def both(call, want):
            got, got_t = call(A), call(t)
            assert isinstance(got, np.ndarray) and got.dtype == out_dtype and np.array_equal(got, want.astype(out_dtype))
            assert got_t.is_cuda and got_t.shape == t.shape and R.same_bytes(got_t.cpu().numpy(), got)

        fp = random_mask((3, 5, 2), 4)
        both(lambda s: volume.median(s), ndi.median_filter(A, size=3, mode="nearest"))
        both(lambda s: volume.median(s, (3, 1, 5), mode="reflect"), ndi.median_filter(A, size=(3, 1, 5), mode="reflect"))
        both(lambda s: volume.median(s, footprint=volume.ball(2), mode="constant", cval=2), ndi.median_filter(A, footprint=volume.ball(2), mode="constant", cval=2))
        both(lambda s: volume.minimum(s, (2, 3, 4), mode="constant", cval=1), ndi.minimum_filter(A, size=(2, 3, 4), mode="constant", cval=1))
        both(lambda s: volume.maximum(s, 5), ndi.maximum_filter(A, size=5, mode="nearest"))
        both(lambda s: volume.minimum(s, footprint=fp), ndi.minimum_filter(A, footprint=fp, mode="nearest"))
        both(lambda s: volume.percentile(s, 30, 3), ndi.percentile_filter(A, 30, size=3, mode="nearest"))
        both(lambda s: volume.percentile(s, -20, footprint=fp, mode="reflect"), ndi.percentile_filter(A, -20, footprint=fp, mode="reflect"))
        both(lambda s: volume.percentile(s, 100, (1, 2, 2)), ndi.percentile_filter(A, 100, size=(1, 2, 2), mode="nearest"))
        both(lambda s: volume.rank_filter(s, 5, 3, origin=(0, 2, 1), mode="reflect"), ndi.rank_filter(A, 5, size=3, mode="reflect", origin=(-1, 1, 0)))
        both(lambda s: volume.rank_filter(s, -3, (4, 2, 3), origin=(3, 0, 1)), ndi.rank_filter(A, -3, size=(4, 2, 3), mode="nearest", origin=(1, -1, 0)))
    # two dimensions and one; bool samples count as uint8
    B = rng.randint(0, 5, size=(23, 70)).astype(np.int16)
    for S, want in ((B, ndi.median_filter(B, size=(3, 5), mode="reflect")), (B[4], ndi.median_filter(B[4], size=5, mode="reflect"))):
        size = (3, 5) if S.ndim == 2 else 5
        assert np.array_equal(volume.median(S, size, mode="reflect"), want)
        got_t = volume.median(torch.from_numpy(S.copy()).cuda(), size, mode="reflect")
        assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy(), want)
    assert np.array_equal(volume.rank_filter(B, 3, footprint=np.array([[1, 0, 1], [1, 1, 1]]), origin=(1, 0)),
                          ndi.rank_filter(B, 3, footprint=np.array([[1, 0, 1], [1, 1, 1]]), mode="nearest", origin=(0, -1)))
    M = rng.uniform(size=(8, 9, 20)) < 0.5
    got = volume.median(M, 3)
    assert got.dtype == np.uint8 and np.array_equal(got, ndi.median_filter(M.astype(np.uint8), size=3, mode="nearest"))
    # for a float type cval is rounded to the sample type first; for an integer type it must be a value of it
    H = (rng.randint(-4, 5, size=(4, 5, 6)) * 0.25).astype(np.float32)
    assert np.array_equal(volume.maximum(H, 3, mode="constant", cval=0.1), ndi.maximum_filter(H, size=3, mode="constant", cval=0.1))
    H16 = H.astype(np.float16)
    assert R.same_bytes(volume.maximum(H16, 3, mode="constant", cval=0.1), R.rank_filter(H16, 26, 3, None, None, "constant", float(np.float16(0.1))))
    for bad in (1.5, -1, 256):
        with pytest.raises(AssertionError):
            volume.median(M, 3, mode="constant", cval=bad)


def _mesh(c, value):
    from contourist_amd import _ffi
    counts = c.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    return counts, c.download_level0_records(counts)


def _same_mesh(a, b):
    (c0, m0), (c1, m1) = a, b
    return c0 == c1 and np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1].view(np.uint32), m1[1].view(np.uint32)) and np.array_equal(m0[2], m1[2])


def test_upload_median_bind_march():
    """a uint8 volume with salt-and-pepper noise is uploaded, its median bound and marched with no copy of the filtered volume on the
    host: the mesh is that of the restatement's median uploaded as uint8"""
    from contourist_amd import _ffi
    A = np.load(os.path.join(GOLDEN_DIR, "noise32_v0.npz"))["A"]
    lo, hi = float(A.min()), float(A.max())
    U = np.clip(np.rint((A - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
    rng = np.random.RandomState(8)
    noise = rng.uniform(size=U.shape)
    U[noise < 0.03], U[noise > 0.97] = 0, 255
    want = R.rank_filter(U, 13, 3)
    assert want.dtype == np.uint8 and not np.array_equal(want, U)
    c, fresh = _ffi.Context(), _ffi.Context()
    try:
        c.upload_grid_native(U)
        before = _ffi.device_bytes(c.handle)[0]
        shape, ptr = c.rank_grid(3, 13)      # the bound grid in, the context's own buffer out
        assert shape == U.shape and c.rank_result() == (U.shape, ptr, "uint8")
        c.bind_ranked()
        assert c.shape == U.shape and c.grid_info() == dict(dtype="uint8", device_bytes=U.size)
        assert _ffi.device_bytes(c.handle)[0] - before <= (1 << 16)      # the noisy grid went; nothing the size of a second copy stays
        fresh.upload_grid_native(want)
        got, ref = _mesh(c, 127.3), _mesh(fresh, 127.3)
        assert _same_mesh(got, ref) and got[0]["n_triangles"] > 1000
    finally:
        c.close()
        fresh.close()


def test_median_of_a_label_mask_feeds_the_distance_transform():
    import distance_ref
    import label_ref
    from contourist_amd import _ffi
    A = field((9, 10, 70), 5)
    labels, k = label_ref.label(A, 0.5, "high", 1)
    keep = np.arange(k + 1) % 3 != 0      # (label 0, the samples without one, is not kept)
    mask = keep[labels].astype(np.uint8)
    cleaned = R.rank_filter(mask, 13, 3)
    assert 0 < cleaned.sum() < mask.sum()
    c = _ffi.Context()
    try:
        assert c.label_grid(0.5, "high", 1, samples=A)[0] == k
        _, mptr = c.label_select(keep)
        _, rptr = c.rank_grid(3, 13, samples=(mptr, "uint8", A.shape))      # the pending mask in, the pending median out
        assert c.rank_result() == (A.shape, rptr, "uint8") and c.label_mask_result()[1] == mptr
        n_sites, dist = c.distance_grid(0.5, "below", "float32", samples=(rptr, "uint8", A.shape), download=True)
        assert n_sites == int(cleaned.sum()) and dist.tobytes() == distance_ref.distance(cleaned, 0.5, "below").tobytes()
        # the result of a call as the input of the next one
        twice = c.rank_grid(3, 13, samples=(rptr, "uint8", A.shape), download=True)[1]
        assert R.same_bytes(twice, R.rank_filter(cleaned, 13, 3))
        _, rptr2 = c.rank_grid(3, 13, samples=(rptr, "uint8", A.shape))
        thrice = c.rank_grid(3, 26, samples=(rptr2, "uint8", A.shape), download=True)[1]
        assert R.same_bytes(thrice, R.rank_filter(R.rank_filter(cleaned, 13, 3), 26, 3))
    finally:
        c.close()


def test_a_call_leaves_the_state_and_binding_resets_it():
    from contourist_amd import _ffi
    A = field((12, 13, 70), 19)
    M, off = np.diag([1.0, 0.5, 1.0]), np.zeros(3)
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)                                                # the other four pending results
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        c.resample_grid(M, off, A.shape)
        res = c.resample_result()
        _, rptr = c.rank_grid(3, 13)                                              # of the bound grid, into the context
        c.rank_grid(3, 0, samples=field((5, 6, 7), 1), download=True)             # of other samples
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts               # the grid is the one uploaded
        levels = c.extract3d_levels([-0.4, 0.1, 0.6], _ffi.CX_DIAG_CPYTHON310)
        c.select_level(1)
        sel = c.download_level0_records(levels[1])
        _, rptr = c.rank_grid((3, 5, 3), 22, mode="reflect")
        assert c.counts() == levels[1]
        assert all(np.array_equal(a, b) for a, b in zip(sel, c.download_level0_records(levels[1])))
        c.select_level(2)
        assert c.counts() == levels[2]
        p = c.postprocess3d()
        # the five pending slots are independent
        assert c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k) and c.resample_result() == res
        filt = c.filter_grid(axes)
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        c.resample_grid(M, off, A.shape)
        res = c.resample_result()
        assert c.rank_result() == (A.shape, rptr, "float32")
        # bind: as after an upload; the other four results stay
        c.bind_ranked()
        for gone in (c.counts, lambda: c.select_level(0), lambda: c.download_level1(p), c.rank_result, c.bind_ranked):
            with pytest.raises(_ffi.CxError) as e:
                gone()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k) and c.resample_result() == res
        assert c.shape == A.shape and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        again = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        fresh = _ffi.Context()
        try:
            fresh.upload_grid(R.rank_filter(A, 22, (3, 5, 3), None, None, "reflect"))
            assert fresh.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == again
        finally:
            fresh.close()
        # the bound grid filtered again, and bound again: the grid owned before is released
        live = _ffi.device_bytes(c.handle)[0]
        c.rank_grid(3, 13)
        c.bind_ranked()
        assert _ffi.device_bytes(c.handle)[0] == live
        # a result with an axis of length 1 is refused and stays pending
        _, rptr = c.rank_grid(3, 4, samples=field((1, 13, 70), 2))
        with pytest.raises(_ffi.CxError) as e:
            c.bind_ranked()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.rank_result() == ((1, 13, 70), rptr, "float32") and c.shape == A.shape
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import torch
    from contourist_amd import _ffi
    A = field((4, 5, 6), 21)

    def code(size=3, rank=0, footprint=None, origin=None, mode="nearest", cval=0, samples=A, **kw):
        with pytest.raises(_ffi.CxError) as e:
            ctx.rank_grid(size, rank, footprint, origin, mode, cval, samples=samples, **kw)
        return e.value.code

    fresh = _ffi.Context()
    try:
        for call in (lambda: fresh.rank_grid(3, 0), fresh.rank_result, fresh.bind_ranked):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
        none = (ctypes_array([3, 3, 3]), ctypes_array([1, 1, 1]))
        assert fresh.lib.cx_grid_rank3d(fresh.handle, None, 0, 1, 0, 0, 0, none[0].ctypes.data, none[1].ctypes.data, None, 0, 0, 0.0, None, None) == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    _ffi.FILTER_MODES["wrap"] = 3
    try:
        assert code(mode="wrap") == _ffi.CX_ERR_INVALID
    finally:
        del _ffi.FILTER_MODES["wrap"]
    for size in ((0, 3, 3), (3, 8, 3), (3, 3, -1), (8, 8, 8)):
        assert code(size=size, origin=(0, 0, 0)) == _ffi.CX_ERR_INVALID
    ctx.rank_grid((7, 7, 7), 342, samples=A)      # the bounds themselves are legal
    ctx.rank_grid((1, 1, 1), 0, samples=A)
    for origin in ((-1, 1, 1), (1, 3, 1), (1, 1, 7)):
        assert code(origin=origin) == _ffi.CX_ERR_INVALID
    ctx.rank_grid((3, 3, 3), 0, origin=(0, 2, 0), samples=A)
    assert code(footprint=np.zeros((3, 3, 3), dtype=bool)) == _ffi.CX_ERR_INVALID
    for rank in (-1, 27, 1 << 20):
        assert code(rank=rank) == _ffi.CX_ERR_INVALID
    five = np.zeros((3, 3, 3), dtype=bool)
    five.reshape(-1)[::6] = True
    assert int(five.sum()) == 5 and code(footprint=five, rank=5) == _ffi.CX_ERR_INVALID
    ctx.rank_grid((3, 3, 3), 4, five, samples=A)
    # cval: finite and a value of the sample type, in every mode
    for cval, mode in itertools.product((float("nan"), float("inf"), -float("inf"), 0.1), R.MODES):
        assert code(cval=cval, mode=mode) == _ffi.CX_ERR_INVALID
    for dtype, cval in ((np.uint8, 1.5), (np.uint8, -1.0), (np.uint8, 256.0), (np.int8, 128.0), (np.uint16, 65536.0), (np.int16, -32769.0),
                        (np.float16, 1.0 + 2.0 ** -11), (np.float16, 65536.0)):
        assert code(samples=np.zeros((2, 3, 4), dtype=dtype), cval=cval, mode="constant") == _ffi.CX_ERR_INVALID, (dtype, cval)
    assert code(samples=(np.zeros(24, dtype=np.uint16), "bfloat16", (2, 3, 4)), cval=1.0 + 2.0 ** -8) == _ffi.CX_ERR_INVALID
    for dtype, cval in ((np.uint8, 255.0), (np.int8, -128.0), (np.float16, 65504.0), (np.float32, 0.5)):
        ctx.rank_grid(3, 1, mode="constant", cval=cval, samples=np.zeros((2, 3, 4), dtype=dtype))
    t = torch.from_numpy(A).cuda()
    torch.cuda.synchronize()
    call = ctx.lib.cx_grid_rank3d
    size, origin = ctypes_array([3, 3, 3]), ctypes_array([1, 1, 1])
    ok = (size.ctypes.data, origin.ctypes.data, None, 0, 0, 0.0, None, None)
    assert call(ctx.handle, t.data_ptr(), 0, 1, 4, 5, 6, *ok) == _ffi.CX_OK
    for dtype in (7, -1):
        assert call(ctx.handle, t.data_ptr(), dtype, 1, 4, 5, 6, *ok) == _ffi.CX_ERR_INVALID
    for shape in ((0, 5, 6), (4, -1, 6), (1 << 16, 1 << 16, 1), (1 << 11, 1 << 11, (1 << 9) + 1)):      # an empty axis, and more than 2^31 samples
        assert call(ctx.handle, t.data_ptr(), 0, 1, shape[0], shape[1], shape[2], *ok) == _ffi.CX_ERR_INVALID
    assert call(None, t.data_ptr(), 0, 1, 4, 5, 6, *ok) == _ffi.CX_ERR_INVALID
    for missing in range(2):
        args = list(ok)
        args[missing] = None
        assert call(ctx.handle, t.data_ptr(), 0, 1, 4, 5, 6, *args) == _ffi.CX_ERR_INVALID
    # an output that overlaps the input: the same memory, its last sample, the sample in front of it
    big = torch.zeros(3 * A.size, dtype=torch.float32, device="cuda")
    inner = big[A.size:2 * A.size]
    inner.copy_(t.reshape(-1))
    torch.cuda.synchronize()
    src = (inner.data_ptr(), inner.dtype, A.shape)
    assert code(samples=src, out=inner.data_ptr()) == _ffi.CX_ERR_INVALID
    assert code(samples=src, out=inner.data_ptr() + 4 * (A.size - 1)) == _ffi.CX_ERR_INVALID
    assert code(samples=src, out=big.data_ptr() + 4) == _ffi.CX_ERR_INVALID
    # next to it is fine
    ctx.rank_grid(3, 13, samples=src, out=big.data_ptr())
    ctx.synchronize()
    assert big[:A.size].cpu().numpy().reshape(A.shape).tobytes() == R.rank_filter(A, 13, 3).tobytes()


def test_a_pointer_into_the_pending_result():
    "planes 1 to 5 of the pending result as the samples of the next call, whose result the context keeps again"
    from contourist_amd import _ffi
    A = field((6, 9, 70), 41, np.uint8)
    first = R.rank_filter(A, 13, 3)
    c = _ffi.Context()
    try:
        _, ptr = c.rank_grid(3, 13, samples=A)
        shape, got = c.rank_grid(3, 13, samples=(ptr + 9 * 70, "uint8", (5, 9, 70)), download=True)
        assert shape == (5, 9, 70) and R.same_bytes(got, R.rank_filter(first[1:], 13, 3))
        assert c.rank_result()[::2] == ((5, 9, 70), "uint8")
    finally:
        c.close()
