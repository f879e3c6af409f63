"""CPU: the numpy restatement of cx_grid_resample3d (tests/resample_ref.py) against what it must equal by construction (identity,
transposes, flips, shifts), against scipy.ndimage.affine_transform, and the map builders of contourist_amd.volume."""
import itertools

import numpy as np
import pytest

import resample_ref as R

EYE = np.eye(3)


def field(shape, seed, dtype=np.float32):
    rng = np.random.RandomState(seed)
    if np.dtype(dtype).kind == "f":
        return (rng.standard_normal(shape) * 3.0).astype(dtype)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=shape).astype(dtype)


def sheared_rotation():
    "the map of the issue's comparison: a 7 x 6 x 9 array into 9 x 8 x 12"
    M = R.rotation((1.0, 2.0, 3.0), 25.0) @ np.array([[0.8, 0.13, 0.0], [0.0, 0.7, 0.21], [0.17, 0.0, 0.75]])
    return R.about_centre(M, (7, 6, 9), (9, 8, 12))


@pytest.mark.parametrize("mode", R.MODES)
def test_identity_reproduces_the_samples(mode):
    A = field((5, 4, 7), 1)
    A[1, 2, 3], A[2, 0, 6], A[4, 3, 0], A[0, 0, 0] = np.inf, -np.inf, np.nan, -0.0
    for order in (0, 1):
        got, n_outside = R.resample(A, EYE, np.zeros(3), A.shape, order, mode, 1.5)
        assert n_outside == 0 and got.dtype == np.float32
        assert got.tobytes() == A.tobytes()
    for dtype in (np.uint8, np.int8, np.uint16, np.int16, np.float16):
        B = field((3, 4, 5), 2, dtype)
        got0, _ = R.resample(B, EYE, np.zeros(3), B.shape, 0, mode, 1.0)
        got1, _ = R.resample(B, EYE, np.zeros(3), B.shape, 1, mode, 1.0)
        assert got0.dtype == B.dtype and got0.tobytes() == B.tobytes()
        assert got1.dtype == np.float32 and np.array_equal(got1, B.astype(np.float32))


def test_bfloat16_bit_patterns():
    f = field((3, 4, 5), 3)
    bits = (f.view(np.uint32) >> 16).astype(np.uint16)
    as_f32 = (bits.astype(np.uint32) << 16).view(np.float32)
    got0, _ = R.resample(bits, EYE, np.zeros(3), bits.shape, 0, "constant", 1.5, dtype="bfloat16")
    got1, _ = R.resample(bits, EYE, np.zeros(3), bits.shape, 1, "constant", 1.5, dtype="bfloat16")
    assert got0.dtype == np.uint16 and np.array_equal(got0, bits) and got1.tobytes() == as_f32.tobytes()
    shifted, n = R.resample(bits, EYE, [0, 0, -1], bits.shape, 0, "constant", 1.5, dtype="bfloat16")
    assert n == 12 and np.all(shifted[:, :, 0] == 0x3FC0) and np.array_equal(shifted[:, :, 1:], bits[:, :, :-1])


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))), ids=lambda p: "".join(map(str, p)))
def test_permutations_and_flips(perm):
    A = field((3, 4, 5), 4)
    want = np.transpose(A, perm)      # want[i] = A[j] with j[perm[k]] = i[k]
    M = np.zeros((3, 3))
    for k in range(3):
        M[perm[k], k] = 1.0
    for order in (0, 1):
        got, n_outside = R.resample(A, M, np.zeros(3), want.shape, order)
        assert n_outside == 0 and got.tobytes() == np.ascontiguousarray(want).tobytes()
        # flipped along every axis of the input
        got, n_outside = R.resample(A, -M, np.asarray(A.shape) - 1.0, want.shape, order)
        assert n_outside == 0 and got.tobytes() == np.ascontiguousarray(want[::-1, ::-1, ::-1]).tobytes()


@pytest.mark.parametrize("order", [0, 1])
def test_integer_offset_is_a_shifted_slice(order):
    A = field((4, 5, 6), 5)
    off = np.array([1.0, -2.0, 3.0])
    got, n_outside = R.resample(A, EYE, off, A.shape, order, "constant", -7.0)
    want = np.full(A.shape, -7.0, dtype=np.float32)
    want[:3, 2:, :3] = A[1:, :3, 3:]
    assert got.tobytes() == want.tobytes() and n_outside == A.size - 3 * 3 * 3
    got, _ = R.resample(A, EYE, off, A.shape, order, "nearest")
    i, j, k = np.meshgrid(*[np.arange(n) for n in A.shape], indexing="ij")
    want = A[np.clip(i + 1, 0, 3), np.clip(j - 2, 0, 4), np.clip(k + 3, 0, 5)]
    assert got.tobytes() == np.ascontiguousarray(want).tobytes()


def test_order_0_needs_an_exact_cval():
    with pytest.raises(AssertionError):
        R.resample(field((2, 2, 2), 1, np.uint8), EYE, np.zeros(3), (2, 2, 2), 0, "constant", 1.5)


SCIPY_MODES = {"nearest": "nearest", "reflect": "reflect", "constant": "grid-constant"}


@pytest.mark.parametrize("mode", R.MODES)
def test_against_scipy(mode):
    ndi = pytest.importorskip("scipy.ndimage")
    A = field((7, 6, 9), 6)
    M, off = sheared_rotation()
    out_shape = (9, 8, 12)
    c = R.coordinates(M, off, out_shape)
    for x in c:      # no coordinate sits on a rounding boundary of order 0, where one ulp decides
        assert np.abs((x + 0.5) - np.rint(x + 0.5)).min() > 1e-9
    assert R.count_outside(c, A.shape) > 100      # the boundary rule is exercised
    got0, _ = R.resample(A, M, off, out_shape, 0, mode, 1.5)
    want0 = ndi.affine_transform(A, M, off, out_shape, order=0, mode=SCIPY_MODES[mode], cval=1.5)
    assert np.array_equal(got0, want0)
    got1, _ = R.resample(A, M, off, out_shape, 1, mode, 1.5)
    want1 = ndi.affine_transform(A.astype(np.float64), M, off, out_shape, order=1, mode=SCIPY_MODES[mode], cval=1.5)
    bound = 2.0 ** -23 * float(np.abs(A).max())      # one fp32 rounding plus float64 noise
    err = float(np.abs(got1.astype(np.float64) - want1).max())
    print("order 1 against scipy, %s: max error %.3g, bound %.3g" % (mode, err, bound))
    assert err <= bound


def test_n_outside_is_counted_on_the_coordinates():
    A = field((4, 4, 4), 7)
    # half a sample beyond the last one on axis 2 only
    _, n = R.resample(A, EYE, [0.0, 0.0, 0.5], A.shape, 1)
    assert n == 16
    _, n = R.resample(A, EYE, [0.0, 0.0, -1e-300], A.shape, 1)
    assert n == 16
    _, n = R.resample(A, np.diag([1.0, 1.0, 3.0 / 7.0]), np.zeros(3), (4, 4, 8), 1)     # the last sample: 7 * (3 / 7) may round above 3
    assert n == (16 if 7 * (3.0 / 7.0) > 3.0 else 0)


# ---- the map builders of contourist_amd.volume (host arithmetic only) --------------------------------------------------------------
def test_zoom_corners_keeps_the_corner_samples():
    from contourist_amd import volume
    A = field((5, 6, 7), 8)
    for factor in (2.0, 0.5, (1.5, 1.0, 3.0)):
        diag, off, out = volume.zoom_map(A.shape, factor, "corners")
        assert out == tuple(int(round(n * f)) for n, f in zip(A.shape, np.ones(3) * factor))
        got, n_outside = R.resample(A, np.diag(diag), off, out, 1)
        for corner in itertools.product((0, -1), repeat=3):
            assert got[corner].tobytes() == A[corner].tobytes()
    # lengths whose plain quotient (n - 1) / (m - 1) falls short of the last sample by a rounding: the step is moved
    for n, m in ((5, 10), (7, 50), (300, 1025)):
        d = volume._corner_scale(n, m)
        assert np.float64(m - 1) * d >= n - 1 and abs(d - (n - 1) / (m - 1)) <= 8 * np.spacing((n - 1) / (m - 1))


def test_zoom_centers_is_scipys_grid_mode():
    ndi = pytest.importorskip("scipy.ndimage")
    from contourist_amd import volume
    A = field((4, 6, 5), 9)
    diag, off, out = volume.zoom_map(A.shape, 2.0, "centers")
    assert out == (8, 12, 10) and np.array_equal(diag, [0.5] * 3) and np.array_equal(off, [-0.25] * 3)
    got, _ = R.resample(A, np.diag(diag), off, out, 1, "nearest")
    want = ndi.zoom(A.astype(np.float64), 2.0, order=1, mode="nearest", grid_mode=True)
    assert np.abs(got - want).max() <= 2.0 ** -23 * float(np.abs(A).max())
    diag, off, out = volume.zoom_map((7,), 1.0 / 3.0)
    assert out == (2,) and diag[0] == 1.0 / (1.0 / 3.0) and off[0] == 0.5 * diag[0] - 0.5


def test_regrid_reproduces_an_affine_function():
    from contourist_amd import volume
    a, b = np.array([0.7, -1.3, 2.1]), 0.4

    def f(shape, mins, delta):
        idx = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
        return sum(a[k] * (mins[k] + delta[k] * idx[k]) for k in range(3)) + b

    mins, delta, shape = np.array([-1.0, 0.5, 2.0]), np.array([0.5, 0.25, 1.25]), (9, 12, 7)
    like_mins, like_delta, like_shape = np.array([-0.3, 0.9, 2.6]), np.array([0.3, 0.2, 0.4]), (10, 9, 14)
    A = f(shape, mins, delta).astype(np.float32)
    for rotation in (None, R.rotation((1.0, 1.0, 0.0), 20.0)):
        M, off = volume.regrid_map(mins, delta, like_shape, like_mins, like_delta, rotation)
        got, n_outside = R.resample(A, M, off, like_shape, 1, "constant", 0.0)
        c = R.coordinates(M, off, like_shape)
        inside = np.ones(like_shape, dtype=bool)
        for k in range(3):
            inside &= (c[k] >= 0.0) & (c[k] <= shape[k] - 1)
        assert n_outside == int((~inside).sum()) and inside.sum() > 200
        # the world point each target index stands for
        x = [mins[k] + delta[k] * c[k] for k in range(3)]
        want = sum(a[k] * x[k] for k in range(3)) + b
        if rotation is None:
            assert np.abs(want - f(like_shape, like_mins, like_delta)).max() < 1e-12
        # each sample carries one fp32 rounding, the result another; the blend of an affine function is exact up to float64 noise
        bound = 2.0 ** -23 * float(np.abs(A).max()) + 1e-9
        assert np.abs(got.astype(np.float64) - want)[inside].max() <= bound


def test_regrid_map_without_rotation_is_a_scaled_identity():
    from contourist_amd import volume
    M, off = volume.regrid_map([0.0, 0.0, 0.0], [1.0, 1.0, 2.5], (4, 4, 10), [0.0, 0.0, 0.0], 1.0)
    assert np.array_equal(M, np.diag([1.0, 1.0, 1.0 / 2.5])) and np.array_equal(off, np.zeros(3))
    new_mins, new_delta = volume.lattice_after([0.0, 0.0, 0.0], [1.0, 1.0, 2.5], M, off)
    assert np.allclose(new_mins, 0.0) and np.allclose(new_delta, 1.0)
    # a transpose with a flip: result axis 0 runs down the samples' axis 2
    P = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-2.0, 0.0, 0.0]])
    new_mins, new_delta = volume.lattice_after([1.0, 2.0, 3.0], [0.1, 0.2, 0.3], P, [0.0, 0.0, 8.0])
    assert np.allclose(new_mins, [3.0 + 0.3 * 8.0, 1.0, 2.0]) and np.allclose(new_delta, [-0.6, 0.1, 0.2])
    with pytest.raises(AssertionError):
        volume.lattice_after([0.0] * 3, 1.0, R.rotation(0, 30.0), np.zeros(3))
