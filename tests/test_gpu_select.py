"""Exact order statistics on the device (cx_samples_select, csrc/cx_pick.hip) against np.sort of the fp32 values: lengths around a
wave and beyond one sweep of the grid-stride loop, misaligned device slices, one bin holding everything, more key prefixes than one
pass refines, NaN / inf / zeros / denormals, every sample type, every shape of rank list, the bound grid, and the 2-D level pickers
with levels_on_device."""
import os

import numpy as np
import pytest

import levels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def ranks_of(n, seed=0, k=12):
    rng = np.random.RandomState(seed)
    r = np.concatenate([[0, n - 1, n // 2], rng.randint(0, n, size=k)]).astype(np.int64)
    return r[rng.permutation(len(r))]


def check(ctx, x, ranks, as_f32=None):
    "select on host samples `x` (numpy) == np.sort; as_f32: the fp32 values where numpy cannot convert x itself"
    from contourist_amd import levels
    got, n_nan = levels.order_statistics(x, ranks, context=ctx)
    want, want_nan = R.select(x if as_f32 is None else as_f32, ranks)
    assert got.dtype == np.float64 and np.array_equal(got, want, equal_nan=True), (got, want)
    assert n_nan == want_nan
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099, 3 * 2 ** 20 + 7])
def test_lengths(ctx, n):
    x = np.random.RandomState(n % 1000).standard_normal(n).astype(np.float32)
    check(ctx, x, ranks_of(n, seed=1))


def test_misaligned_device_slices(ctx):
    import torch
    for dtype, np_dtype, off in ((torch.float32, np.float32, 1), (torch.uint8, np.uint8, 1), (torch.int16, np.int16, 3), (torch.float32, np.float32, 3)):
        rng = np.random.RandomState(off)
        host = rng.standard_normal(5000).astype(np_dtype) if np_dtype is np.float32 else rng.randint(-100, 100, size=5000).astype(np_dtype)
        t = torch.from_numpy(host).cuda()[off:]
        assert t.data_ptr() % 16 != 0
        check_tensor(ctx, t, host[off:], ranks_of(len(host) - off, seed=2))


def check_tensor(ctx, t, host_f32_source, ranks):
    from contourist_amd import levels
    got, n_nan = levels.order_statistics(t, ranks, context=ctx)
    want, want_nan = R.select(host_f32_source, ranks)
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    assert n_nan == want_nan


def test_one_bin_holds_everything(ctx):
    x = np.full(2 ** 18 + 3, 1.25, dtype=np.float32)
    check(ctx, x, [0, len(x) - 1, 12345])
    y = np.where(np.arange(2 ** 22 + 5) % 3 == 0, np.float32(-2.5), np.float32(7.0)).astype(np.float32)
    n_low = int((y == -2.5).sum())
    got = check(ctx, y, [0, n_low - 1, n_low, len(y) - 1])
    assert list(got) == [-2.5, -2.5, 7.0, 7.0] and n_low > 2 ** 16


def test_more_prefixes_than_one_pass(ctx):
    rng = np.random.RandomState(5)
    n = 60000
    x = (np.where(rng.rand(n) < 0.5, -1.0, 1.0) * np.ldexp(1.0 + rng.rand(n), rng.randint(-30, 31, size=n))).astype(np.float32)
    ranks = np.linspace(0, n - 1, 96).astype(np.int64)
    got = check(ctx, x, ranks)
    assert len(set((R.key_f32(got.astype(np.float32)) >> 21).tolist())) >= 40


def test_special_values(ctx):
    x = R.special_field()
    n = len(x)
    ranks = np.concatenate([np.arange(0, n, 7), np.arange(n - 60, n)])
    got = check(ctx, x, ranks)
    assert np.isnan(got[-8:]).all() and np.isposinf(got[-9]) and np.isneginf(got[0])
    from contourist_amd import levels
    assert levels.order_statistics(x, [0], context=ctx)[1] == 8
    assert np.array_equal(levels.quantiles(x, [0.0, 1.0]), [-np.inf, np.inf])      # over the samples that are not NaN


@pytest.mark.parametrize("name", ["float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16"])
def test_dtypes(ctx, name):
    rng = np.random.RandomState(11)
    n = 20011
    if name == "uint8":
        x = np.concatenate([np.arange(256), rng.randint(0, 256, size=n)]).astype(np.uint8)
    elif name == "int8":
        x = np.concatenate([np.arange(-128, 128), rng.randint(-128, 128, size=n)]).astype(np.int8)
    elif name == "uint16":
        x = np.concatenate([[0, 65535, 32768, 32767], rng.randint(0, 65536, size=n)]).astype(np.uint16)
    elif name == "int16":
        x = np.concatenate([[-32768, 32767, -1, 0], rng.randint(-32768, 32768, size=n)]).astype(np.int16)
    elif name in ("float16", "bfloat16"):
        x = (rng.standard_normal(n) * 100).astype(np.float16)
        x[:8] = np.array([np.nan, -np.nan, -0.0, 0.0, np.inf, -np.inf, 6e-8, -6e-8], dtype=np.float16)      # (6e-8: a half denormal)
        x.view(np.uint16)[8] = 0xFE01                                                                          # a negative NaN with a payload
    else:
        x = rng.standard_normal(n).astype(np.float32)
    ranks = np.concatenate([ranks_of(len(x), seed=3, k=40), np.arange(0, len(x), 997)])
    if name == "bfloat16":
        import torch
        t = torch.from_numpy(x.astype(np.float32)).cuda().to(torch.bfloat16)
        t[5000] = float("nan")
        t[5001] = -0.0
        check_tensor(ctx, t, t.float().cpu().numpy(), ranks)
    else:
        got = check(ctx, x, ranks)
        if name == "uint8":
            assert np.array_equal(np.unique(check(ctx, x, np.arange(0, len(x), 20))), np.arange(256, dtype=np.float64))
        if name in ("int8", "int16"):
            assert got.min() < 0


def test_rank_lists(ctx):
    x = np.random.RandomState(13).standard_normal(30011).astype(np.float32)
    n = len(x)
    check(ctx, x, [n - 1, 0])
    check(ctx, x, [17])
    check(ctx, x, [500, 3, 500, 29000, 3, 3, n - 1, 0, 500])
    check(ctx, x, np.random.RandomState(14).randint(0, n, size=1024))


def test_bound_grid_and_errors(ctx):
    from contourist_amd import _ffi
    rng = np.random.RandomState(17)
    for A in (rng.randint(0, 256, size=(9, 10, 11)).astype(np.uint8), rng.standard_normal((9, 10, 11)).astype(np.float32)):
        ctx.upload_grid_native(A)
        ranks = ranks_of(A.size, seed=4)
        got, n_nan = ctx.samples_select(ranks)
        want, _ = R.select(A, ranks)
        assert np.array_equal(got, want) and n_nan == 0
    x = rng.standard_normal(100).astype(np.float32)
    for bad in ([100], [0, -1], []):
        with pytest.raises(_ffi.CxError) as e:
            ctx.samples_select(bad, x)
        assert e.value.code == _ffi.CX_ERR_INVALID
    fresh = _ffi.Context()
    try:
        with pytest.raises(_ffi.CxError) as e:
            fresh.samples_select([0])
        assert e.value.code == _ffi.CX_ERR_STATE
    finally:
        fresh.close()


def test_extraction_survives(ctx):
    from contourist_amd import _ffi
    A = np.random.RandomState(19).standard_normal((12, 13, 70)).astype(np.float32)
    ctx.upload_grid(A)
    c = ctx.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
    before = ctx.download_level0_records(c)
    check(ctx, np.random.RandomState(20).standard_normal(70000).astype(np.float32), ranks_of(70000, seed=5))
    got, _ = ctx.samples_select([0, A.size - 1])
    assert list(got) == [float(A.min()), float(A.max())]
    assert ctx.counts() == c
    after = ctx.download_level0_records(c)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_2d_level_pickers_on_device():
    from conftest import ROOT
    from contourist_amd import multiple_2d_contour
    A = np.load(os.path.join(ROOT, "tests", "golden2d", "percentile_36x31.npz"))["A"]
    n, m = A.shape

    def f(x, y):
        return A[np.rint(x).astype(int), np.rint(y).astype(int)]

    for cls in (multiple_2d_contour.Percentile2DContour, multiple_2d_contour.Linear2DContour):
        for breakpoints in (5, 10):
            args = (0, 0, n - 1 + 0.25, m - 1 + 0.25, 1, 1, f)
            host = cls(*args, breakpoints=breakpoints)
            dev = cls(*args, breakpoints=breakpoints, levels_on_device=True)
            assert len(host.values) >= 4
            assert [float(v).hex() for v in dev.values] == [float(v).hex() for v in host.values]
