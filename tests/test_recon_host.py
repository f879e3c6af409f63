"""CPU: the numpy restatement of cx_grid_reconstruct3d (tests/recon_ref.py) against independent statements of the same thing -- the
sequential raster / anti-raster algorithm, scipy's binary propagation and fill-holes, plateaus found by labelling, the duality of the
two methods, the special values of the floats -- and the argument checks of the contourist_amd.volume helpers, which need no GPU."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import rank_ref as R
import recon_ref as C

CONNECTIVITIES = (1, 2, 3)


def grey(shape, seed, levels=5, dtype=np.uint8):
    "few distinct values: ties everywhere"
    return np.random.RandomState(seed).randint(0, levels, size=shape).astype(dtype)


def marker_below(mask, seed, above=0.1):
    "the mask minus random amounts, and some samples above it (those are clamped)"
    rng = np.random.RandomState(seed)
    g = mask.astype(np.int64) - rng.randint(0, 4, size=mask.shape) * (rng.uniform(size=mask.shape) < 0.8)
    g = np.where(rng.uniform(size=mask.shape) < above, mask.astype(np.int64) + 2, g)
    info = np.iinfo(mask.dtype)
    return np.clip(g, info.min, info.max).astype(mask.dtype)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_iterate_equals_the_sequential_sweeps(connectivity):
    for seed, shape in enumerate([(4, 5, 6), (1, 7, 9), (3, 3, 3), (2, 1, 11)]):
        F = R.key(grey(shape, seed))
        G = np.minimum(R.key(marker_below(grey(shape, seed), 50 + seed)), F)
        assert np.array_equal(C.iterate(G, F, connectivity), C.raster(G, F, connectivity))
        # the result is a fixed point between the marker and the mask
        V = C.iterate(G, F, connectivity)
        assert np.all(V >= G) and np.all(V <= F) and np.array_equal(np.minimum(F, C.dilate(V, connectivity)), V)


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_binary_inputs_equal_scipys_propagation(connectivity):
    rng = np.random.RandomState(connectivity)
    mask = rng.uniform(size=(7, 8, 9)) < {1: 0.45, 2: 0.25, 3: 0.15}[connectivity]      # (denser, and everything is one component)
    seeds = mask & (rng.uniform(size=mask.shape) < 0.1)
    want = ndi.binary_propagation(seeds, ndi.generate_binary_structure(3, connectivity), mask=mask)
    got, n_changed, n_clamped = C.reconstruct(mask.astype(np.uint8), seeds.astype(np.uint8), connectivity=connectivity)
    assert np.array_equal(got, want.astype(np.uint8)) and n_clamped == 0 and n_changed == int(mask.sum() - want.sum())
    assert 0 < want.sum() < mask.sum()


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_erosion_from_the_rim_fills_the_holes_of_a_mask(connectivity):
    rng = np.random.RandomState(10 + connectivity)
    mask = ndi.binary_dilation(rng.uniform(size=(9, 10, 11)) < 0.12, ndi.generate_binary_structure(3, 1))
    mask[2:7, 3:8, 4:9] = True
    mask[3:6, 4:7, 5:8] = False      # a closed box: a hole at every connectivity
    want = ndi.binary_fill_holes(mask, ndi.generate_binary_structure(3, connectivity))
    got = C.reconstruct(mask.astype(np.uint8), "rim", method="erosion", connectivity=connectivity)[0]
    assert np.array_equal(got, want.astype(np.uint8))
    assert want.sum() > mask.sum()


def plateau_maxima(A, connectivity):
    "1 on the plateaus (components of A == v) that have no higher neighbour"
    st = ndi.generate_binary_structure(3, connectivity)
    out = np.zeros(A.shape, dtype=np.uint8)
    higher = ndi.maximum_filter(A, footprint=st, mode="nearest") > A
    for v in np.unique(A):
        labels, k = ndi.label(A == v, st)
        for c in range(1, k + 1):
            if not higher[labels == c].any():
                out[labels == c] = 1
    return out


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_regional_maxima_are_the_plateaus_without_a_higher_neighbour(connectivity):
    for seed, dtype in ((1, np.uint8), (2, np.int16), (3, np.float32)):
        A = grey((6, 7, 8), seed, 4, np.int64).astype(dtype) - (2 if dtype != np.uint8 else 0)
        got = C.reconstruct(A, "step", connectivity=connectivity, out_kind="changed")[0]
        assert np.array_equal(got, plateau_maxima(A, connectivity)) and 0 < got.sum() < A.size
        low = C.reconstruct(A, "step", method="erosion", connectivity=connectivity, out_kind="changed")[0]
        assert np.array_equal(low, plateau_maxima(-A.astype(np.float64), connectivity))


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_erosion_is_dilation_of_the_complement(connectivity):
    F = grey((5, 6, 7), 4, 6)
    G = marker_below(F, 5)
    for kind in (G, "step", "rim"):
        a = C.reconstruct(F, kind, faces=5, method="dilation", connectivity=connectivity)
        b = C.reconstruct(255 - F, kind if isinstance(kind, str) else 255 - G, faces=5, method="erosion", connectivity=connectivity)
        assert np.array_equal(a[0], 255 - b[0]) and a[1:] == b[1:]
    a = C.reconstruct(F, "shift", h=2, method="dilation", connectivity=connectivity)
    b = C.reconstruct(255 - F, "shift", h=2, method="erosion", connectivity=connectivity)
    assert np.array_equal(a[0], 255 - b[0]) and a[1] == b[1] and a[1] > 0


def test_the_constant_extreme_of_an_integer_type_is_one_extremum():
    for A, method in ((np.zeros((2, 3, 4), np.uint8), "dilation"), (np.full((2, 3, 4), -128, np.int8), "dilation"), (np.full((2, 3, 4), 255, np.uint8), "erosion")):
        got, n_changed, _ = C.reconstruct(A, "step", method=method, out_kind="changed")
        assert got.all() and n_changed == 0
        assert np.array_equal(C.reconstruct(A, "step", method=method)[0], A)
    # any other constant is one extremum by the rule itself
    assert C.reconstruct(np.full((2, 3, 4), 7, np.uint8), "step", out_kind="changed")[0].all()


def bits32(*patterns):
    return np.array(patterns, dtype=np.uint32).view(np.float32).reshape(1, 1, -1)


def test_special_float_values():
    inf = np.float32(np.inf)
    # -0.0 lies below +0.0: beside each other, +0.0 is the maximum and -0.0 the minimum
    Z = np.array([0.0, -0.0, -0.0, 0.0], dtype=np.float32).reshape(1, 1, 4)
    assert C.reconstruct(Z, "step", out_kind="changed")[0].reshape(-1).tolist() == [1, 0, 0, 1]
    assert C.reconstruct(Z, "step", method="erosion", out_kind="changed")[0].reshape(-1).tolist() == [0, 1, 1, 0]
    # the steps saturate at the infinities; NaN steps down to +inf and stays under erosion
    K = R.key(np.array([-inf, inf, np.nan, 0.0, -0.0], dtype=np.float32))
    down, up = C.step_keys(K, "float32", "dilation"), C.step_keys(K, "float32", "erosion")
    assert down.tolist() == [K[0], K[1] - 1, K[1], K[4], K[4] - 1] and up.tolist() == [K[0] + 1, K[1], K[2], K[3] + 1, K[3]]
    # NaN is the top of the order: it is a regional maximum, lets everything pass as a mask, and comes out canonical
    N = bits32(0x3F800000, 0xFFC12345, 0x40000000, 0x7F800000)      # 1, a negative NaN with a payload, 2, +inf
    assert C.reconstruct(N, "step", out_kind="changed")[0].reshape(-1).tolist() == [0, 1, 0, 1]
    assert C.reconstruct(bits32(0x7F800000, 0xFFC12345, 0x40000000), "step", out_kind="changed")[0].reshape(-1).tolist() == [0, 1, 0]
    got = C.reconstruct(N, bits32(0xFF800000, 0xFF800000, 0xFF800000, 0x7F800000))[0]
    assert got.view(np.uint32).reshape(-1).tolist() == [0x3F800000, 0x40000000, 0x40000000, 0x7F800000]
    got = C.reconstruct(N, bits32(0xFF800000, 0x7FFFFFFF, 0xFF800000, 0xFF800000))[0]
    assert got.view(np.uint32).reshape(-1).tolist() == [0x3F800000, 0x7FC00000, 0x40000000, 0x40000000]
    # h-maxima: infinities stay, a NaN stays, the sum is rounded once
    H = np.array([inf, 1.0, -inf, np.nan, 3.0, 1.0 + 2.0 ** -23], dtype=np.float32).reshape(1, 1, -1)
    G = C.shift_keys(H, "float32", 0.5, "dilation")
    assert R.unkey(G, "float32").view(np.uint32).reshape(-1).tolist() == np.array([inf, 0.5, -inf, np.nan, 2.5, 0.5 + 2.0 ** -23], dtype=np.float32).view(np.uint32).tolist()
    # float16 and bfloat16: one rounding from float64, ties to even
    h16 = np.array([1.0, 2048.0, 65504.0], dtype=np.float16).reshape(1, 1, -1)
    assert R.unkey(C.shift_keys(h16, "float16", 2.0 ** -11, "erosion"), "float16").reshape(-1).tolist() == [1.0, 2048.0, 65504.0]
    assert R.unkey(C.shift_keys(h16, "float16", 3 * 2.0 ** -11, "erosion"), "float16").reshape(-1).tolist() == [1.0 + 2.0 ** -9, 2048.0, 65504.0]
    assert np.isinf(R.unkey(C.shift_keys(h16, "float16", 16.0, "erosion"), "float16").reshape(-1)[2])
    b16 = np.array([0x3F80, 0x4300, 0x7F7F], dtype=np.uint16).reshape(1, 1, -1)      # 1, 128, the largest finite value
    assert R.unkey(C.shift_keys(b16, "bfloat16", 2.0 ** -8, "erosion"), "bfloat16").reshape(-1).tolist() == [0x3F80, 0x4300, 0x7F7F]
    assert R.unkey(C.shift_keys(b16, "bfloat16", 3 * 2.0 ** -8, "erosion"), "bfloat16").reshape(-1).tolist() == [0x3F82, 0x4300, 0x7F7F]
    assert R.unkey(C.shift_keys(b16, "bfloat16", 2.0 ** 120, "erosion"), "bfloat16").reshape(-1).tolist()[2] == 0x7F80
    assert C.round_bfloat16([1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8), 2.0 ** -133, 0.0]).tolist() == [0x3F81, 0xBF80, 0x0001, 0x0000]


def test_shift_saturates_in_integer_types():
    for dtype in (np.uint8, np.int8, np.int16, np.uint16):
        info = np.iinfo(dtype)
        A = np.array([info.min, info.min + 1, 0, info.max - 1, info.max], dtype=dtype).reshape(1, 1, -1)
        down = R.unkey(C.shift_keys(A, A.dtype.name, 3, "dilation"), A.dtype.name).reshape(-1)
        up = R.unkey(C.shift_keys(A, A.dtype.name, 3, "erosion"), A.dtype.name).reshape(-1)
        assert down.tolist() == [info.min, info.min, max(info.min, -3), info.max - 4, info.max - 3]
        assert up.tolist() == [info.min + 3, info.min + 4, 3, info.max, info.max]
        assert R.unkey(C.shift_keys(A, A.dtype.name, 1e6, "dilation"), A.dtype.name).reshape(-1).tolist() == [info.min] * 5


def test_volume_helpers_check_their_arguments():
    "every check comes before the first call into the library, so no GPU is needed to fail it"
    from contourist_amd import volume
    U = grey((3, 4, 5), 1)
    F = U.astype(np.float32)
    bad = [lambda: volume.h_maxima(U, 1.5), lambda: volume.h_maxima(U, 0), lambda: volume.h_minima(F, -1.0), lambda: volume.h_domes(F, float("nan")),
           lambda: volume.h_basins(F, float("inf")), lambda: volume.h_maxima(U, 1, connectivity=4), lambda: volume.regional_maxima(U, connectivity=0),
           lambda: volume.reconstruct(U, U, method="opening"), lambda: volume.reconstruct(U[:2], U), lambda: volume.reconstruct(F, U),
           lambda: volume.reconstruct("step", U), lambda: volume.clear_border_grey(U, faces=0), lambda: volume.clear_border_grey(U, faces=64),
           lambda: volume.clear_border_grey(U[0], faces=16), lambda: volume.clear_border_grey(U, faces="rim"), lambda: volume.propagate(F, U),
           lambda: volume.propagate(U, F), lambda: volume.regional_minima(np.zeros((2, 2, 2, 2), np.uint8))]
    for n, call in enumerate(bad):
        with pytest.raises(AssertionError):
            call()
    assert volume._recon_faces("all", 3) == 63 and volume._recon_faces("all", 2) == 60 and volume._recon_faces(3, 1) == 48
    assert volume._recon_h(2, np.uint8) == 2.0 and volume._recon_h(0.25, np.float16) == 0.25 and volume._recon_h(0.25, "torch.bfloat16") == 0.25
