"""CPU: the numpy restatement of the isovalue pickers (tests/levels_ref.py) against itself (difference arrays vs. a brute-force
classifier per level), against the reference's recorded counts (tests/golden/*.npz), against np.sort (the key order) and against the
values of the existing 2-D level pickers; and the host-side rank rules of contourist_amd/levels.py."""
import os

import numpy as np
import pytest

import levels_ref as R
from conftest import GOLDEN_DIR

CLEAN = ("blobs27", "inv_sphere20", "noise24_v0", "noise24_v07", "noise24_v07_smooth03", "noise32_v0", "noise32_vm05", "noise_14x20x26",
         "shells24", "sphere32", "sphere32_smooth05")
NEAR = ("quantised18", "rel_tol16", "tiny_amp16", "tiny_amp16b")


def golden(name):
    return np.load(os.path.join(GOLDEN_DIR, name + ".npz"))


def noise(shape, seed, nan=0):
    rng = np.random.RandomState(seed)
    A = rng.standard_normal(shape).astype(np.float32)
    for _ in range(nan):
        A[tuple(rng.randint(0, n) for n in shape)] = np.nan
    return A


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in R.KEYS)


@pytest.mark.parametrize("shape,nan", [((5, 4, 3), 0), ((2, 2, 2), 0), ((14, 20, 26), 0), ((5, 4, 3), 3), ((14, 20, 26), 5)])
def test_difference_arrays_equal_brute_force(shape, nan):
    A = noise(shape, 7 + nan, nan)
    finite = A[np.isfinite(A)]
    values = [0.3, -0.7, 0.3, 0.0, float(finite[0]), float(finite.min()) - 1.0, float(finite.max()) + 1.0, 1.1, -2.0, 0.3]   # unsorted, duplicates, a sample itself
    got, want = R.spectrum(A, values), R.spectrum_brute(A, values)
    assert same(got, want), (got, want)
    assert got["n_cells"][5] == 0 and got["n_vertices"][5] == 0 and got["n_triangles"][5] == 0      # below the minimum: nothing is low
    if nan == 0:
        assert got["n_cells"][6] == 0 and got["n_vertices"][6] == 0      # above the maximum all is low -- but for a NaN, which never is
    assert got["n_near"][4] >= 1
    assert np.array_equal(got["n_cells"][[0, 2, 9]], got["n_cells"][[0, 0, 0]])


def test_many_levels_equal_single_levels():
    A = golden("noise_14x20x26")["A"]
    values = np.linspace(-2.1, 2.1, 336)
    assert same(R.spectrum(A, values), R.spectrum_brute(A, values))


@pytest.mark.parametrize("name", CLEAN)
def test_counts_of_the_reference(name):
    z = golden(name)
    got = R.spectrum(z["A"], [float(z["value"])])
    assert got["n_near"][0] == 0
    assert (got["n_cells"][0], got["n_vertices"][0], got["n_triangles"][0]) == (len(z["surface_voxels"]), len(z["l0_pairs"]), len(z["l0_tris"]))


def test_noise32_v0_figures():
    z = golden("noise32_v0")
    got = R.spectrum(z["A"], [0.0])
    assert (got["n_cells"][0], got["n_vertices"][0], got["n_triangles"][0]) == (11793, 37040, 74288)


@pytest.mark.parametrize("name", NEAR)
def test_fixtures_inside_the_screen(name):
    z = golden(name)
    assert R.spectrum(z["A"], [float(z["value"])])["n_near"][0] > 0


def test_key_order_is_sort_order():
    x = R.special_field()
    keys = R.key_f32(x)
    by_key = x[np.argsort(keys, kind="stable")]
    assert np.array_equal(by_key, np.sort(x), equal_nan=True)       # (-0.0 == +0.0: either may stand)
    assert int((keys == 0xFFFFFFFF).sum()) == int(np.isnan(x).sum()) == 8
    # equal keys only for equal values (and for the NaNs)
    s = np.sort(x)
    ks = np.sort(keys)
    assert np.array_equal(ks[1:] == ks[:-1], (s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1])))
    for k in (0x007FFFFF, 0x7FFFFFFE, 0x80000000, 0x80000001, 0xFF800000):
        assert int(R.key_f32(R.unkey_f32(k))[0]) == k


def test_screen_bounds_hold_the_screen():
    for value in (0.0, 1.0, -3.7, 100.0, 1e-30, 3e38):
        vcmp, near = R.value_params(value)
        lo, hi = R.screen_bounds(vcmp, near)
        assert R._inside(lo, vcmp, near) and R._inside(hi, vcmp, near)
        assert not R._inside(lo - 1, vcmp, near) and not R._inside(hi + 1, vcmp, near)


def test_level_rules_equal_the_2d_classes():
    from contourist_amd import levels, multiple_2d_contour, triangulated

    def f(x, y):
        return np.sin(3.0 * x) * y + 0.25 * x

    for breakpoints in (4, 5, 10):
        P = multiple_2d_contour.Percentile2DContour(-1, -1, 1, 1, 0.1, 0.07, f, breakpoints=breakpoints)
        L = multiple_2d_contour.Linear2DContour(-1, -1, 1, 1, 0.1, 0.07, f, breakpoints=breakpoints)
        lattice = triangulated.grid_lattice(P.function_grid)[2]
        assert lattice.dtype == np.float32
        want = R.percentile_values(lattice, breakpoints)
        assert [float(v).hex() for v in want] == [float(v).hex() for v in P.values]
        assert [float(v).hex() for v in R.linear_values(lattice, breakpoints)] == [float(v).hex() for v in L.values]
        # the rank rules of the device path pick the same samples
        ranks = levels.percentile_ranks(lattice.size, breakpoints)
        picked = np.sort(lattice, axis=None)[ranks].astype(np.float64)
        assert [float(v).hex() for v in picked] == [float(v).hex() for v in P.values]
        assert P.levels_on_device is False and L.levels_on_device is False


def test_quantile_ranks():
    from contourist_amd import levels
    x = noise((9, 8, 7), 5, nan=4).reshape(-1)
    n_valid = int((~np.isnan(x)).sum())
    q = [0.0, 0.1, 0.5, 0.9, 1.0, 0.3333]
    ranks = levels.quantile_ranks(q, n_valid)
    assert np.array_equal(np.sort(x)[ranks], np.nanquantile(x, q, method="lower"))
    assert ranks[0] == 0 and ranks[4] == n_valid - 1
