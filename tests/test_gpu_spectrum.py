"""The per-level size curve on the device (cx_level_spectrum3d, csrc/cx_pick.hip) against tests/levels_ref.py, bit for bit in all four
arrays, and against the march itself wherever no sample lies inside a level's tolerance screen."""
import os

import numpy as np
import pytest

import levels_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

CLEAN = ("blobs27", "inv_sphere20", "noise24_v0", "noise24_v07", "noise24_v07_smooth03", "noise32_v0", "noise32_vm05", "noise_14x20x26",
         "shells24", "sphere32", "sphere32_smooth05")


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def smooth(shape, seed, passes=2):
    B = np.random.RandomState(seed).standard_normal(shape)
    for _ in range(passes):
        for ax in range(3):
            B = 0.25 * np.roll(B, 1, ax) + 0.5 * B + 0.25 * np.roll(B, -1, ax)
    return (B / B.std()).astype(np.float32)


def fields():
    rng = np.random.RandomState(23)
    I, J, K = np.meshgrid(np.arange(32), np.arange(32), np.arange(32), indexing="ij")
    with_nan = rng.standard_normal((9, 11, 70)).astype(np.float32)
    with_nan[rng.randint(0, 9, 12), rng.randint(0, 11, 12), rng.randint(0, 70, 12)] = np.nan
    with_nan[8, 10, 69] = np.nan
    return {
        "2x2x2": rng.standard_normal((2, 2, 2)).astype(np.float32),
        "5x4x3": rng.standard_normal((5, 4, 3)).astype(np.float32),
        "noise_14x20x26": rng.standard_normal((14, 20, 26)).astype(np.float32),
        "smooth_33x17x66": smooth((33, 17, 66), 24),
        "smooth_65x9x130": smooth((65, 9, 130), 25),
        "checkerboard32": np.where((I + J + K) % 2 == 0, np.float32(1.0), np.float32(-1.0)).astype(np.float32),
        "uint8_12x13x67": rng.randint(0, 256, size=(12, 13, 67)).astype(np.uint8),
        "int16_7x9x65": rng.randint(-3000, 3000, size=(7, 9, 65)).astype(np.int16),
        "nan_9x11x70": with_nan,
    }


FIELDS = fields()


def level_sets(name, A):
    f = A.astype(np.float32)
    lo, hi = float(np.nanmin(f)), float(np.nanmax(f))
    rng = np.random.RandomState(len(name))
    span = hi - lo
    sets = {
        "one": [0.5 * (lo + hi)],
        "mixed": [lo + 0.3 * span, hi + 1.0, lo + 0.3 * span, lo - 1.0, float(f.flat[1]), lo + 0.71 * span, lo, hi, 0.0],      # duplicates, unsorted, outside, samples themselves
        "many": list(rng.uniform(lo - 0.05 * span, hi + 0.05 * span, size=300)),
    }
    if name == "uint8_12x13x67":
        sets["half_steps"] = [k + 0.5 for k in range(-1, 256)]
        sets["integers"] = [float(k) for k in range(0, 256, 5)]
    if name == "checkerboard32":
        sets["zero"] = [0.0]
    if name in ("smooth_33x17x66", "nan_9x11x70"):
        sets["4096"] = list(np.linspace(lo - 0.1, hi + 0.1, 4093)) + [0.0, 0.0, float(f.flat[5])]
    return sets


def same(got, want):
    assert set(got) == set(R.KEYS)
    for k in R.KEYS:
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_parity_with_the_restatement(ctx, name):
    A = FIELDS[name]
    ctx.upload_grid_native(A)
    assert ctx.grid_info()["dtype"] == A.dtype.name
    for label, values in level_sets(name, A).items():
        got = ctx.level_spectrum3d(values)
        want = R.spectrum(A, values)
        same(got, want)
        if label == "mixed":
            assert got["n_cells"][3] == 0 and got["n_vertices"][3] == 0 and got["n_triangles"][3] == 0 and got["n_near"][3] == 0
            if not np.isnan(A.astype(np.float32)).any():
                assert got["n_vertices"][1] == 0 and got["n_near"][1] == 0
            assert got["n_near"][4] >= 1 and np.array_equal(got["n_cells"][[0]], got["n_cells"][[2]])
        if label == "zero":
            n = 32
            assert got["n_cells"][0] == (n - 1) ** 3 and got["n_near"][0] == 0
            assert got["n_vertices"][0] == 3 * n * n * (n - 1) + (n - 1) ** 3       # the axis edges and the body diagonals cross; the face diagonals join equal signs
        again = ctx.level_spectrum3d(values)
        same(again, got)


def test_equals_the_march_on_noise(ctx):
    from contourist_amd import _ffi
    A = np.load(os.path.join(GOLDEN_DIR, "noise_14x20x26.npz"))["A"]
    ctx.upload_grid(A)
    values = np.linspace(-1.5, 1.5, 16) + 3e-3      # (no sample of the fixture inside any of the 16 screens: the restatement says so)
    assert np.all(R.spectrum(A, values)["n_near"] == 0)
    got = ctx.level_spectrum3d(values)
    assert np.all(got["n_near"] == 0)
    for l, v in enumerate(values):
        c = ctx.extract3d(float(v), _ffi.CX_DIAG_CPYTHON310)
        assert (c["n_cells"], c["n_vertices"], c["n_triangles"]) == (got["n_cells"][l], got["n_vertices"][l], got["n_triangles"][l]), (v, c)


@pytest.mark.parametrize("name", CLEAN)
def test_equals_the_march_on_goldens(ctx, name):
    from contourist_amd import _ffi
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    A, v = z["A"], float(z["value"])
    f = A.astype(np.float32)
    others = np.random.RandomState(31).uniform(float(f.min()) - 0.1, float(f.max()) + 0.1, size=300)
    values = np.concatenate([others[:137], [v], others[137:]])
    ctx.upload_grid_native(A)
    got = ctx.level_spectrum3d(values)
    assert got["n_near"][137] == 0
    c = ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
    assert (c["n_cells"], c["n_vertices"], c["n_triangles"]) == (got["n_cells"][137], got["n_vertices"][137], got["n_triangles"][137])
    assert (c["n_cells"], c["n_vertices"], c["n_triangles"]) == (len(z["surface_voxels"]), len(z["l0_pairs"]), len(z["l0_tris"]))


def test_extraction_and_selected_level_survive(ctx):
    from contourist_amd import _ffi
    A = FIELDS["smooth_33x17x66"]
    ctx.upload_grid(A)
    c = ctx.extract3d(0.2, _ffi.CX_DIAG_CPYTHON310)
    before = ctx.download_level0_records(c)
    ctx.level_spectrum3d(np.linspace(-1, 1, 50))
    assert ctx.counts() == c
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.download_level0_records(c)))
    counts = ctx.extract3d_levels([-0.4, 0.1, 0.6], _ffi.CX_DIAG_CPYTHON310)
    ctx.select_level(1)
    before = ctx.download_level0_records(counts[1])
    got = ctx.level_spectrum3d([-0.4, 0.1, 0.6])
    assert ctx.counts() == counts[1]
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.download_level0_records(counts[1])))
    ctx.select_level(2)
    assert ctx.counts() == counts[2]
    # this surface runs into the upper faces of the array, where the march also keeps a record for every lattice point that owns a
    # crossing edge but no whole cell: its n_cells is larger there, its n_border_voxels is the number of whole cells
    assert np.all(got["n_near"] == 0)
    for l in range(3):
        assert (counts[l]["n_border_voxels"], counts[l]["n_vertices"], counts[l]["n_triangles"]) == (got["n_cells"][l], got["n_vertices"][l], got["n_triangles"][l])
        assert counts[l]["n_cells"] >= got["n_cells"][l]


def test_errors():
    from contourist_amd import _ffi
    fresh = _ffi.Context()
    try:
        with pytest.raises(_ffi.CxError) as e:
            fresh.level_spectrum3d([0.0])
        assert e.value.code == _ffi.CX_ERR_STATE
        fresh.upload_grid(FIELDS["5x4x3"])
        for bad in ([], [0.0] * 4097, [float("nan")], [float("inf")], [1e39]):
            with pytest.raises(_ffi.CxError) as e:
                fresh.level_spectrum3d(bad)
            assert e.value.code == _ffi.CX_ERR_INVALID
    finally:
        fresh.close()


def test_python_surface():
    from contourist_amd import levels, tetrahedral
    A = FIELDS["smooth_33x17x66"]
    values = [0.6, -0.3, 0.1]
    want = R.spectrum(A, values)
    same(levels.spectrum(A, values), want)
    M = tetrahedral.MultiLevelIsosurfaces(None, None, None, A, values)
    got = M.spectrum()
    same(got, R.spectrum(A, sorted(values)))
    same(M.spectrum([0.25]), R.spectrum(A, [0.25]))
    q = [0.2, 0.5, 0.9]
    Q = tetrahedral.MultiLevelIsosurfaces.at_quantiles(None, None, None, A, q)
    assert Q.values == sorted(float(v) for v in np.quantile(A.reshape(-1), q, method="lower"))
