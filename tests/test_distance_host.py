"""The restatement of cx_grid_distance3d (tests/distance_ref.py) against scipy.ndimage on the host: what the GPU tests compare the device
with bit for bit is itself the Euclidean distance transform."""
import numpy as np
import pytest

import distance_ref as R

SHAPES = [(2, 2, 2), (5, 4, 3), (9, 70, 131), (37, 33, 259)]
DENSITIES = [0.5, 0.03, 0.001]
SAMPLINGS = [(2.5, 1.0, 0.7), (0.3, 0.3, 1.25)]


def random_sites(shape, density, seed):
    rng = np.random.RandomState(seed)
    sites = rng.uniform(size=shape) < density
    sites.reshape(-1)[rng.randint(sites.size)] = True      # at least one: scipy returns garbage without a site
    return sites


@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unit_sampling_is_scipy_bit_for_bit(shape, density):
    nd = pytest.importorskip("scipy.ndimage")
    sites = random_sites(shape, density, 1)
    d2 = R.transform(sites)
    s = nd.distance_transform_edt(~sites)
    assert np.array_equal(d2, np.rint(s * s))
    assert np.array_equal(np.sqrt(d2).view(np.uint64), s.view(np.uint64))


@pytest.mark.parametrize("sampling", SAMPLINGS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sampling_within_4_ulps_of_scipy(shape, sampling):
    """scipy sums its three terms in another order than the per-axis minimum does.  Measured with scipy 1.15.3 on these shapes, densities
    and samplings: the worst difference is 2 float64 ulps ((37, 33, 259) at density 0.001); 1 ulp on every other case."""
    nd = pytest.importorskip("scipy.ndimage")
    for density in DENSITIES:
        sites = random_sites(shape, density, 1)
        a = np.sqrt(R.transform(sites, sampling))
        s = nd.distance_transform_edt(~sites, sampling=sampling)
        ulps = int(np.abs(a.view(np.int64) - s.view(np.int64)).max())
        print(shape, sampling, density, "ulps:", ulps)
        assert ulps <= 4


def test_sides_and_signed():
    A = np.random.RandomState(2).standard_normal((6, 7, 9)).astype(np.float32)
    parts = R.both(A, 0.2)
    gA, gB = parts
    low = A < 0.2
    assert np.all(gA[low] == 0) and np.all(gA[~low] > 0) and np.all(gB[~low] == 0) and np.all(gB[low] > 0)
    assert np.array_equal(R.squared(A, 0.2, "signed"), R.squared(A, 0.2, "above") - R.squared(A, 0.2, "below"))
    sd = R.distance(A, 0.2, "signed")
    assert sd.dtype == np.float32 and np.array_equal(sd, (np.sqrt(gA) - np.sqrt(gB)).astype(np.float32))
    assert np.array_equal(sd, R.distance(A, 0.2, "above") - R.distance(A, 0.2, "below"))      # one of the two is 0 everywhere
    assert np.all((sd < 0) == low) and not np.any(sd == 0)
    nd = pytest.importorskip("scipy.ndimage")
    assert np.array_equal(R.distance(A, 0.2, "below"), nd.distance_transform_edt(A < 0.2).astype(np.float32))
    assert np.array_equal(R.distance(A, 0.2, "above"), nd.distance_transform_edt(A >= 0.2).astype(np.float32))


def test_no_site_is_infinite():
    A = np.zeros((3, 4, 5), dtype=np.float32)
    assert np.all(np.isposinf(R.squared(A, -1.0, "above"))) and np.all(R.squared(A, -1.0, "below") == 0)
    assert np.all(np.isposinf(R.distance(A, -1.0, "signed"))) and np.all(np.isneginf(R.distance(A, 1.0, "signed")))
    assert not R.mask(A, -1.0, "above", 1e300).any()
    assert R.n_sites(A, -1.0, "above") == 0 and R.n_sites(A, -1.0, "below") == 60 and R.n_sites(A, -1.0, "signed") == 0


def test_low_rule():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    A = np.asarray([nan, -inf, inf, -0.0, 0.0], dtype=np.float32)
    assert R.low_mask(A, 0.0).tolist() == [False, True, False, False, False]      # -0.0 < 0.0 is false, a NaN is never low
    assert R.low_mask(A, -0.0).tolist() == [False, True, False, False, False]
    assert R.low_mask(A, 5e-324).tolist() == [False, True, False, True, True]
    # a value between two float32 neighbours: the comparison is made in float64, the value is not rounded to float32
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(2.0))
    value = (np.float64(a) + np.float64(b)) / 2
    assert np.float32(value) in (a, b)
    assert R.low_mask(np.asarray([a, b]), value).tolist() == [True, False]
    assert R.low_mask(np.asarray([a, b]), np.float64(b)).tolist() == [True, False]
    assert R.low_mask(np.asarray([a, b]), np.nextafter(np.float64(b), 2.0)).tolist() == [True, True]


def ball(radius, sampling=(1.0, 1.0, 1.0)):
    "the digitised ball: the offsets whose squared length, summed as the transform sums it, is <= radius^2"
    w = R.weights(sampling)
    r = [int(np.floor(radius / np.sqrt(w[a]))) + 1 for a in range(3)]
    z, y, x = np.meshgrid(*[np.arange(-n, n + 1) for n in r], indexing="ij")
    d2 = (w[2] * x ** 2 + w[1] * y ** 2) + w[0] * z ** 2
    return d2 <= np.float64(radius) * np.float64(radius)


@pytest.mark.parametrize("radius", [1.0, 1.5, 2.0, 3.0])
def test_morphology_is_scipys(radius):
    nd = pytest.importorskip("scipy.ndimage")
    X = np.random.RandomState(3).uniform(size=(11, 12, 20)) < 0.3
    X[4:9, 3:9, 5:15] = True
    B = ball(radius)
    dil = lambda S: nd.binary_dilation(S, structure=B)      # (outside the array: background)
    ero = lambda S: ~dil(~S)                               # nothing outside the array erodes the set
    M = X.astype(np.uint8)
    assert np.array_equal(R.dilate(M, 0.5, radius).astype(bool), dil(X))
    assert np.array_equal(R.erode(M, 0.5, radius).astype(bool), ero(X))
    assert np.array_equal(R.opened(M, 0.5, radius).astype(bool), dil(ero(X)))
    assert np.array_equal(R.closed(M, 0.5, radius).astype(bool), ero(dil(X)))
    assert R.dilate(M, 0.5, radius).dtype == np.uint8
    # opening shrinks, closing grows, and both are idempotent
    o, c = R.opened(M, 0.5, radius), R.closed(M, 0.5, radius)
    assert np.all(o <= M) and np.all(c >= M)
    assert np.array_equal(R.opened(o, 0.5, radius), o) and np.array_equal(R.closed(c, 0.5, radius), c)


def test_morphology_with_sampling():
    nd = pytest.importorskip("scipy.ndimage")
    sampling = (2.0, 1.0, 0.5)      # squares exact in float64: the ball's sums are too
    X = np.random.RandomState(4).uniform(size=(9, 10, 21)) < 0.2
    B = ball(2.0, sampling)
    assert np.array_equal(R.dilate(X.astype(np.uint8), 0.5, 2.0, sampling).astype(bool), nd.binary_dilation(X, structure=B))
