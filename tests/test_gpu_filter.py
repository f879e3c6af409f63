"""cx_grid_filter3d (csrc/cx_filter.hip) against its numpy restatement (tests/filter_ref.py), bit for bit: shapes around the kernels'
tiles (a wave owns 64 columns of axis 2 and 16 outputs of the walked axis, axis 1 in the first kernel and axis 0 in the second), the
three boundary rules, weight shapes, strides, every sample type from the host and from a device tensor, misaligned device slices, a
caller's output, NaN and infinite samples, contourist_amd.volume, the end-to-end route upload -> filter -> bind -> march with no host
copy, what a filter call leaves alone and what a bind resets, and the error codes."""
import os

import numpy as np
import pytest

import filter_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# 2 x 16 + 5 planes, 2 x 16 + 1 rows, 4 x 64 + 3 columns: the last chunk of either walk is partial (5 planes, 1 row), the last tile of
# columns holds 3, and with the kernels below every wave of the first two chunks reads rows and planes that belong to its neighbours
STRADDLE = (37, 33, 259)


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


def weights(n, seed, normalised=True):
    w = np.random.RandomState(seed).uniform(0.1, 1.0, size=n)
    return (w / w.sum() if normalised else w).astype(np.float32)


def check(ctx, A, axes, mode="nearest", cval=0.0, as_f32=None, samples=None):
    "the device result of host samples A (or of `samples`) == the restatement on A (as_f32: its float32 values), bit for bit"
    shape, got = ctx.filter_grid(axes, mode, cval, samples=A if samples is None else samples, download=True)
    want = R.filter3d(A if as_f32 is None else as_f32, axes, mode, cval)
    assert got.dtype == np.float32 and shape == want.shape == got.shape, (shape, want.shape)
    assert not np.isnan(want).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    return got


SHAPES = [(2, 2, 2), (1, 8, 9), (5, 4, 3), (3, 5, 63), (3, 5, 64), (2, 6, 65), (2, 3, 131), STRADDLE]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_and_modes(ctx, shape, mode):
    A = field(shape, 11)
    if shape == (2, 2, 2):      # radius 10: the positions run through five reflections of the axis
        axes = [(weights(21, a), 10, 1) for a in range(3)]
    else:
        axes = [(weights(5, 1), 2, 1), (weights(3, 2), 1, 1), (weights(9, 3), 4, 1)]
    check(ctx, A, axes, mode, 1.5)


WEIGHT_CASES = {
    "radius_per_axis": [(weights(7, 1), 3, 1), (None, 0, 1), (weights(3, 2), 1, 1)],
    "only_axis_0": [(weights(5, 1), 2, 1), (None, 0, 1), (None, 0, 1)],
    "none_at_all": [(None, 0, 1), (None, 0, 1), (None, 0, 1)],
    "one_weight": [(np.asarray([0.75], dtype=np.float32), 0, 1)] * 3,
    "129_weights": [(weights(129, 4), 64, 1), (weights(129, 5), 64, 1), (weights(129, 6), 64, 1)],
    "32_and_33_weights": [(weights(32, 4), 16, 1), (weights(33, 5), 16, 1), (weights(32, 6), 0, 1)],      # the most the walk's window of 32 rows takes, and one more
    "33_and_32_weights": [(weights(33, 4), 0, 1), (weights(32, 5), 31, 1), (weights(33, 6), 32, 1)],
    "even_origin_0": [(weights(4, 7), 0, 1), (weights(6, 8), 0, 1), (weights(8, 9), 0, 1)],
    "even_origin_last": [(weights(4, 7), 3, 1), (weights(6, 8), 5, 1), (weights(8, 9), 7, 1)],
    "antisymmetric": [(np.asarray([-0.5, 0.0, 0.5], dtype=np.float32), 1, 1), (np.asarray([-1.0, 1.0], dtype=np.float32), 0, 1),
                      (np.asarray([1.0, -8.0, 0.0, 8.0, -1.0], dtype=np.float32) / 12, 2, 1)],
}


@pytest.mark.parametrize("case", sorted(WEIGHT_CASES))
def test_weight_shapes(ctx, case):
    A = field((19, 21, 70), 5)
    A[3, 4, 5] = -0.0      # an axis that is not filtered keeps its bits
    for mode in R.MODES:
        check(ctx, A, WEIGHT_CASES[case], mode, 1.5)


def test_segments_too_long_to_stage(ctx):
    "63 stride + taps samples under a wave's columns go through LDS up to 256 of them: 255 (staged) and 318, 192 + 65 (read from memory)"
    A = field((4, 18, 300), 23)
    for taps, stride in ((129, 2), (129, 3), (65, 3), (66, 3)):
        w = weights(taps, taps)
        for mode in R.MODES:
            check(ctx, A, [(None, 0, 1), (weights(3, 1), 1, 1), (w, taps // 2, stride)], mode, 1.5)
            check(ctx, A, [(weights(3, 1), 1, 1), (w[:17], 8, stride), (w, taps // 2, stride)], mode, 1.5)


@pytest.mark.parametrize("strides", [(2, 2, 2), (2, 3, 1), (3, 1, 2), "axis_length"], ids=str)
def test_strides(ctx, strides):
    shape = (18, 21, 140)
    A = field(shape, 6)
    st = shape if strides == "axis_length" else strides
    kernels = {
        "taps_overlap": [weights(5, 1), weights(7, 2), weights(9, 3)],      # more taps than the stride: neighbours share samples
        "taps_apart": [weights(2, 1), weights(1, 2), weights(2, 3)],        # at most as many taps as the stride (where it is > 1)
        "window_shrinks": [weights(17, 1), weights(31, 2), weights(9, 3)],  # fewer than 16 outputs per wave keep the walked samples within 32 rows
        "no_taps": [None, None, None],
        "mixed": [None, weights(4, 2), None],
    }
    for name, rows in kernels.items():
        axes = [(w, 0 if w is None else len(w) // 2, s) for w, s in zip(rows, st)]
        for mode in R.MODES:
            got = check(ctx, A, axes, mode, 1.5)
            assert got.shape == tuple(-(-n // s) for n, s in zip(shape, st)), name
    if strides == (2, 2, 2):
        B = field(STRADDLE, 8)
        check(ctx, B, [(weights(5, 1), 2, 2), (weights(5, 2), 2, 2), (weights(5, 3), 2, 2)], "reflect")
        # the strided result is the unstrided one subsampled
        full = ctx.filter_grid([(weights(5, a), 2, 1) for a in range(3)], "reflect", samples=A, download=True)[1]
        part = ctx.filter_grid([(weights(5, a), 2, 2) for a in range(3)], "reflect", samples=A, download=True)[1]
        assert np.array_equal(part.view(np.uint32), full[::2, ::2, ::2].view(np.uint32))


@pytest.mark.parametrize("name", ["float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16"])
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    shape = (7, 18, 67)
    axes = [(weights(3, 1), 1, 1), (weights(5, 2), 2, 2), (weights(7, 3), 3, 1)]
    if name == "bfloat16":
        t = torch.from_numpy(field(shape, 9)).cuda().to(torch.bfloat16)
        f32 = t.float().cpu().numpy()
        host = (t.view(torch.int16).cpu().numpy().view(np.uint16), "bfloat16", shape)
    else:
        A = field(shape, 9, np.dtype(name))
        if name.startswith(("int", "uint")):
            info = np.iinfo(A.dtype)
            A[0, 0, :2] = [info.min, info.max]
        t = torch.from_numpy(A).cuda()
        f32, host = A.astype(np.float32), A
    torch.cuda.synchronize()
    for mode in ("reflect", "constant"):
        a = check(ctx, f32, axes, mode, 1.5, samples=host)
        b = check(ctx, f32, axes, mode, 1.5, samples=(t.data_ptr(), t.dtype, shape))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_misaligned_device_slice_and_callers_output(ctx):
    import torch
    shape = (5, 9, 71)
    n = int(np.prod(shape))
    axes = [(weights(3, 1), 1, 2), (weights(5, 2), 2, 1), (weights(7, 3), 3, 1)]
    for np_dtype, off in ((np.float32, 1), (np.uint8, 1), (np.int16, 3), (np.uint8, 7)):
        flat = field(n + off, off + 20, np_dtype)
        t = torch.from_numpy(flat).cuda()[off:]
        assert t.data_ptr() % 16 != 0
        A = flat[off:].reshape(shape)
        want = R.filter3d(A, axes, "reflect")
        out = torch.full((int(np.prod(want.shape)) + 2,), -7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        got_shape, ptr = ctx.filter_grid(axes, "reflect", samples=(t.data_ptr(), t.dtype, shape), out=out[1:].data_ptr())
        ctx.synchronize()
        host = out.cpu().numpy()
        assert got_shape == want.shape and ptr == out[1:].data_ptr()
        assert host[0] == -7.0 and host[-1] == -7.0      # nothing written around the result
        assert np.array_equal(host[1:-1].view(np.uint32), want.reshape(-1).view(np.uint32))
        # with an output of the caller's the context holds no result
        from contourist_amd import _ffi
        with pytest.raises(_ffi.CxError) as e:
            ctx.filter_result()
        assert e.value.code == _ffi.CX_ERR_STATE


def test_nan_and_infinite_samples(ctx):
    A = field((9, 12, 70), 13)
    A[2, 3, 4], A[5, 6, 60], A[7, 1, 33] = np.nan, np.inf, -np.inf
    A[5, 6, 66] = -np.inf      # meets the +inf under the 9 taps of axis 2: inf - inf
    axes = [(weights(3, 1), 1, 1), (weights(5, 2), 2, 1), (weights(9, 3), 4, 1)]
    for mode in R.MODES:
        with np.errstate(all="ignore"):
            want = R.filter3d(A, axes, mode, 1.5)
        got = ctx.filter_grid(axes, mode, 1.5, samples=A, download=True)[1]
        assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        keep = ~np.isnan(want)
        assert np.array_equal(got.view(np.uint32)[keep], want.view(np.uint32)[keep])


def test_volume_module(ctx):
    import torch
    from contourist_amd import volume
    A = field((20, 33, 70), 15)
    U = field((20, 33, 70), 16, np.uint8)
    for S in (A, U):
        assert R.same_bits(volume.gaussian(S, 1.0), R.gaussian(S, 1.0))
        assert R.same_bits(volume.gaussian(S, (0.0, 2.5, 0.6), stride=(1, 2, 1), mode="reflect"), R.gaussian(S, (0.0, 2.5, 0.6), stride=(1, 2, 1), mode="reflect"))
        assert R.same_bits(volume.gaussian(S, 16.0, mode="constant", cval=1.5), R.gaussian(S, 16.0, mode="constant", cval=1.5))      # 129 taps
        assert R.same_bits(volume.block_mean(S, 2), R.block_mean(S, 2))
        assert R.same_bits(volume.block_mean(S, (3, 1, 4), mode="reflect"), R.block_mean(S, (3, 1, 4), mode="reflect"))      # partial last blocks
        got, want = volume.pyramid(S, 4), R.pyramid(S, 4)
        assert got[0] is S and [g.shape for g in got] == [(20, 33, 70), (10, 17, 35), (5, 9, 18), (3, 5, 9)]
        assert all(R.same_bits(g, w) for g, w in zip(got[1:], want[1:]))
    # a tensor in, a tensor out; two dimensions and one
    t = torch.from_numpy(U).cuda()
    out = volume.gaussian(t, 1.0, stride=2)
    assert out.is_cuda and out.dtype == torch.float32 and R.same_bits(out.cpu().numpy(), R.gaussian(U, 1.0, stride=2))
    pyr = volume.pyramid(t, 3)
    assert pyr[0] is t and all(R.same_bits(g.cpu().numpy(), w) for g, w in zip(pyr[1:], R.pyramid(U, 3)[1:]))
    B = A[3]
    assert R.same_bits(volume.gaussian(B, (1.0, 2.0)), R.gaussian(B[None], (0.0, 1.0, 2.0))[0])
    assert R.same_bits(volume.block_mean(B[5], 4), R.block_mean(B[5][None, None], (1, 1, 4))[0, 0])
    w = weights(6, 3, normalised=False)
    assert R.same_bits(volume.convolve_separable(A, w, strides=(1, 2, 3), origins=(0, 5, 2), mode="constant", cval=-1.0),
                       R.filter3d(A, [(w, 0, 1), (w, 5, 2), (w, 2, 3)], "constant", -1.0))
    # float64 samples are rounded to float32 first
    assert R.same_bits(volume.gaussian(A.astype(np.float64) + 1e-12, 1.0), R.gaussian((A.astype(np.float64) + 1e-12).astype(np.float32), 1.0))


def test_two_calls_give_the_same_bits(ctx):
    A = field(STRADDLE, 17)
    axes = [(weights(9, 1), 4, 1), (weights(9, 2), 4, 2), (weights(9, 3), 4, 1)]
    a = ctx.filter_grid(axes, "reflect", samples=A, download=True)[1]
    ctx.filter_grid([(None, 0, 1)] * 3, samples=field((3, 3, 3), 1), download=True)      # (the scratch is reused in between)
    b = ctx.filter_grid(axes, "reflect", samples=A, download=True)[1]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_upload_filter_bind_march(ctx):
    """a uint8 volume is uploaded, smoothed and marched with no float32 copy on the host: the mesh is that of the restatement's result
    uploaded as float32"""
    from contourist_amd import _ffi, volume
    A = np.load(os.path.join(GOLDEN_DIR, "noise32_v0.npz"))["A"]
    lo, hi = float(A.min()), float(A.max())
    U = np.clip(np.rint((A - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
    w = volume.gaussian_weights(1.0)
    axes = [(w, len(w) // 2, 1)] * 3
    want = R.gaussian(U, 1.0)
    value = 127.3
    meshes = []
    for route in ("device", "host"):
        c = _ffi.Context()
        try:
            if route == "device":
                c.upload_grid_native(U)
                assert c.grid_info() == dict(dtype="uint8", device_bytes=U.size)
                shape, ptr = c.filter_grid(axes)      # the bound grid in, the context's own buffer out
                assert shape == U.shape and c.filter_result() == (shape, ptr)
                c.bind_filtered()
                assert c.shape == shape
            else:
                c.upload_grid(want)
            assert c.grid_info() == dict(dtype="float32", device_bytes=want.size * 4)
            counts = c.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
            meshes.append((counts, c.download_level0_records(counts)))
        finally:
            c.close()
    (c0, m0), (c1, m1) = meshes
    assert c0 == c1 and c0["n_triangles"] > 1000
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1].view(np.uint32), m1[1].view(np.uint32)) and np.array_equal(m0[2], m1[2])


def test_filtering_leaves_the_state_and_binding_resets_it():
    from contourist_amd import _ffi
    A = field((12, 13, 70), 19)
    axes = [(weights(3, a), 1, 1) for a in range(3)]
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        c.filter_grid(axes)                                                       # of the bound grid, into the context
        c.filter_grid(axes, samples=field((5, 6, 7), 1), download=True)           # of other samples
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts               # the grid is the one uploaded
        levels = c.extract3d_levels([-0.4, 0.1, 0.6], _ffi.CX_DIAG_CPYTHON310)
        c.select_level(1)
        sel = c.download_level0_records(levels[1])
        c.filter_grid(axes)
        assert c.counts() == levels[1]
        assert all(np.array_equal(a, b) for a, b in zip(sel, c.download_level0_records(levels[1])))
        c.select_level(2)
        assert c.counts() == levels[2]
        p = c.postprocess3d()
        # bind: as after an upload
        shape, _ = c.filter_grid(axes)
        c.bind_filtered()
        for gone in (c.counts, lambda: c.select_level(0), lambda: c.download_level1(p), c.filter_result, c.bind_filtered):
            with pytest.raises(_ffi.CxError) as e:
                gone()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert c.shape == shape == A.shape
        again = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        fresh = _ffi.Context()
        try:
            fresh.upload_grid(R.filter3d(A, axes))
            assert fresh.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == again
        finally:
            fresh.close()
        # the bound grid filtered again, and bound again: the grid owned before is released
        live = _ffi.device_bytes(c.handle)[0]
        c.filter_grid(axes)
        c.bind_filtered()
        assert _ffi.device_bytes(c.handle)[0] == live
        # a result the march does not take stays pending
        c.filter_grid([(None, 0, 12), (None, 0, 1), (None, 0, 1)])
        with pytest.raises(_ffi.CxError) as e:
            c.bind_filtered()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.filter_result()[0] == (1, 13, 70) and c.shape == A.shape
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    from contourist_amd import _ffi
    A = field((4, 5, 6), 21)
    ok = (weights(3, 1), 1, 1)

    def code(axes, mode="nearest", cval=0.0, samples=A, **kw):
        with pytest.raises(_ffi.CxError) as e:
            ctx.filter_grid(axes, mode, cval, samples=samples, **kw)
        return e.value.code

    fresh = _ffi.Context()
    try:
        for call in (lambda: fresh.filter_grid([ok] * 3), fresh.filter_result, fresh.bind_filtered):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    bad_axes = [
        (np.zeros(130, dtype=np.float32), 64, 1),      # more than 129 weights
        (weights(3, 1), 3, 1), (weights(3, 1), -1, 1),      # origin outside 0 .. n_weights-1
        (weights(3, 1), 1, 0), (weights(3, 1), 1, 7), (None, 0, 0), (None, 0, 7),      # stride outside 1 .. n
    ]
    for bad in bad_axes:
        for axis in range(3):
            axes = [ok] * 3
            axes[axis] = bad
            assert code(axes) == _ffi.CX_ERR_INVALID, (bad[1:], axis)
    _ffi.FILTER_MODES["wrap"] = 3
    try:
        assert code([ok] * 3, mode="wrap") == _ffi.CX_ERR_INVALID
    finally:
        del _ffi.FILTER_MODES["wrap"]
    for cval in (float("nan"), float("inf"), -float("inf")):
        assert code([ok] * 3, cval=cval) == _ffi.CX_ERR_INVALID
        assert code([ok] * 3, mode="constant", cval=cval) == _ffi.CX_ERR_INVALID
    import torch
    t = torch.from_numpy(A).cuda()
    torch.cuda.synchronize()
    dev = (t.data_ptr(), t.dtype, A.shape)
    rc = ctx.lib.cx_grid_filter3d(ctx.handle, t.data_ptr(), 7, 1, 4, 5, 6, None, 0, 0.0, None, None, None)
    assert rc == _ffi.CX_ERR_INVALID      # no axes
    recs = (_ffi.cx_filter_axis * 3)()
    for r in recs:
        r.stride = 1
    import ctypes
    for dtype in (7, -1):
        assert ctx.lib.cx_grid_filter3d(ctx.handle, t.data_ptr(), dtype, 1, 4, 5, 6, ctypes.cast(recs, ctypes.c_void_p), 0, 0.0, None, None, None) == _ffi.CX_ERR_INVALID
    assert ctx.lib.cx_grid_filter3d(ctx.handle, t.data_ptr(), 0, 1, 0, 5, 6, ctypes.cast(recs, ctypes.c_void_p), 0, 0.0, None, None, None) == _ffi.CX_ERR_INVALID
    # an output that overlaps the input: the same memory, its last sample, the sample in front of it
    assert code([ok] * 3, samples=dev, out=t.data_ptr()) == _ffi.CX_ERR_INVALID
    assert code([ok] * 3, samples=dev, out=t.data_ptr() + 4 * (A.size - 1)) == _ffi.CX_ERR_INVALID
    big = torch.zeros(3 * A.size, dtype=torch.float32, device="cuda")
    inner = big[A.size:2 * A.size]
    inner.copy_(t.reshape(-1))
    torch.cuda.synchronize()
    assert code([ok] * 3, samples=(inner.data_ptr(), inner.dtype, A.shape), out=big.data_ptr() + 4) == _ffi.CX_ERR_INVALID
    # next to it is fine
    shape, ptr = ctx.filter_grid([ok] * 3, samples=(inner.data_ptr(), inner.dtype, A.shape), out=big.data_ptr())
    ctx.synchronize()
    assert np.array_equal(big[:A.size].cpu().numpy().reshape(shape).view(np.uint32), R.filter3d(A, [ok] * 3).view(np.uint32))


def test_offsets_beyond_32_bits(ctx):
    """2^30 float32 samples (4 GB): the byte offsets of the second half do not fit 32 bits.  Strides of a quarter axis keep 2 x 4 x 4
    outputs; each is restated from the few samples under its taps."""
    import torch
    n0, n1, n2 = 2, 1 << 14, 1 << 15
    flat = torch.arange(n0 * n1 * n2, dtype=torch.int32, device="cuda").remainder_(8191).float()

    def sample(i, j, k):
        return np.float32(((i * n1 + j) * n2 + k) % 8191)

    w1, w2 = weights(2, 1), weights(3, 2)
    axes = [(None, 0, 1), (w1, 0, n1 // 4), (w2, 1, n2 // 4)]
    torch.cuda.synchronize()
    shape, got = ctx.filter_grid(axes, "reflect", samples=(flat.data_ptr(), flat.dtype, (n0, n1, n2)), download=True)
    assert shape == (2, 4, 4)
    for i in range(2):
        for a in range(4):
            for b in range(4):
                rows = []
                for t1 in range(2):
                    j = int(R.src(a * (n1 // 4) + t1, n1, "reflect")[0])
                    acc = np.float64(0.0)
                    for t2 in range(3):
                        k = int(R.src(b * (n2 // 4) + t2 - 1, n2, "reflect")[0])
                        acc = acc + np.float64(w2[t2]) * np.float64(sample(i, j, k))
                    rows.append(np.float32(acc))
                acc = np.float64(0.0)
                for t1 in range(2):
                    acc = acc + np.float64(w1[t1]) * np.float64(rows[t1])
                assert np.float32(acc).view(np.uint32) == got[i, a, b].view(np.uint32), (i, a, b)


def three_taps(seed):
    return (weights(3, seed), 1, 1)


# the pending result fed back as `samples`, the new result kept in the context again.  Axis 0 not filtered: one kernel, which before
# the step-aside read and wrote the same buffer; all axes: two kernels; stride 2: the output is smaller than the input
CHAIN_CASES = {
    "one_kernel": [(None, 0, 1), three_taps(1), three_taps(2)],
    "two_kernels": [three_taps(0), three_taps(1), three_taps(2)],
    "one_kernel_stride_2": [(None, 0, 1), three_taps(1), (weights(3, 2), 1, 2)],
    "two_kernels_stride_2": [three_taps(0), three_taps(1), (weights(3, 2), 1, 2)],
}


@pytest.mark.parametrize("case", sorted(CHAIN_CASES))
def test_the_pending_result_is_the_next_input(case):
    "axis 2 (70) is longer than one tile of 64 columns; every step == the restatement applied once more; steady state allocates nothing"
    from contourist_amd import _ffi
    axes = CHAIN_CASES[case]
    A = field((5, 9, 70), 31)
    c = _ffi.Context()
    try:
        shape, ptr = c.filter_grid(axes, "reflect", samples=A)
        want = R.filter3d(A, axes, "reflect")
        assert shape == want.shape
        for step in range(2, 6):
            if step >= 4:      # from the third chained call on (the fourth call in all)
                before = _ffi.device_bytes(c.handle)
            shape, got = c.filter_grid(axes, "reflect", samples=(ptr, "float32", shape), download=True)
            want = R.filter3d(want, axes, "reflect")
            assert shape == want.shape == got.shape, (step, shape, want.shape)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (step, float(np.abs(got - want).max()))
            described, ptr = c.filter_result()
            assert described == shape and ptr
            if step >= 4:
                assert _ffi.device_bytes(c.handle) == before, step
    finally:
        c.close()
