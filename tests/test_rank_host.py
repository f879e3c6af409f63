"""tests/rank_ref.py, the numpy restatement of cx_grid_rank3d, against scipy.ndimage's rank filters on NaN-free data, its keys and its
order on the special values, and the helpers of contourist_amd.volume that choose a rank or a footprint.  No GPU."""
import itertools

import numpy as np
import pytest
import scipy.ndimage as ndi

import levels_ref
import rank_ref as R

SCIPY_MODES = {"nearest": "nearest", "reflect": "reflect", "constant": "constant"}


def tied(shape, seed, dtype):
    "few distinct values: every window holds ties"
    rng = np.random.RandomState(seed)
    if np.dtype(dtype).kind == "f":
        return (rng.randint(-4, 5, size=shape) * 0.25).astype(dtype)
    lo = -3 if np.dtype(dtype).kind == "i" else 0
    return rng.randint(lo, lo + 7, size=shape).astype(dtype)


def ends_and_centre(box):
    return [tuple(0 for s in box), tuple(s // 2 for s in box), tuple(s - 1 for s in box)]


def scipy_origin(box, origin):
    return [o - s // 2 for s, o in zip(box, origin)]


def random_mask(box, seed):
    rng = np.random.RandomState(seed)
    fp = rng.uniform(size=box) < 0.6
    fp.reshape(-1)[rng.randint(fp.size)] = True
    return fp


# ---- the keys ---------------------------------------------------------------------------------------------------------------------------

def test_keys_of_the_special_values_fp32():
    x = levels_ref.special_field()
    k = R.key(x)
    u = x.view(np.uint32)
    nan = np.isnan(x)
    assert k.dtype == np.uint32 and nan.sum() == 8
    assert np.all(k[nan] == 0xFFFFFFFF) and np.all(k[~nan] != 0xFFFFFFFF)
    back = R.unkey(k, "float32").view(np.uint32)
    assert np.array_equal(back[~nan], u[~nan]) and np.all(back[nan] == 0x7FC00000)
    # the order of the keys is the order of the values, and -0.0 comes before +0.0
    order = np.argsort(k[~nan], kind="stable")
    v = x[~nan][order]
    assert np.all(v[:-1] <= v[1:])
    kz = R.key(np.array([-0.0, 0.0], dtype=np.float32))
    assert kz[0] + 1 == kz[1]
    smallest = np.array([0x80000001, 0x80000000, 0x00000000, 0x00000001], dtype=np.uint32).view(np.float32)      # -denormal, -0, +0, +denormal
    assert np.all(np.diff(R.key(smallest).astype(np.int64)) == 1)
    ends = R.key(np.array([-np.inf, -3.4028235e38, 3.4028235e38, np.inf], dtype=np.float32)).astype(np.int64)
    assert np.all(np.diff(ends) > 0) and ends[3] < 0xFFFFFFFF and ends[1] - ends[0] == 1 and ends[3] - ends[2] == 1


@pytest.mark.parametrize("name", ["float16", "bfloat16"])
def test_keys_of_the_special_values_16_bits(name):
    _, _, inf, qnan = R.FLOATS[name]
    u = np.arange(1 << 16, dtype=np.uint16)      # every bit pattern
    k = R.key(u if name == "bfloat16" else u.view(np.float16), "bfloat16" if name == "bfloat16" else None)
    nan = (u & 0x7FFF) > inf
    assert np.all(k[nan] == 0xFFFF) and len(np.unique(k[~nan])) == int((~nan).sum()) and np.all(k[~nan] != 0xFFFF)
    back = R.unkey(k, name).view(np.uint16)
    assert np.array_equal(back[~nan], u[~nan]) and np.all(back[nan] == qnan)
    wide = (u.astype(np.uint32) << 16).view(np.float32) if name == "bfloat16" else u.view(np.float16).astype(np.float32)
    v = wide[~nan][np.argsort(k[~nan], kind="stable")]
    assert np.all(v[:-1] <= v[1:])
    assert k[0x8000] + 1 == k[0x0000] and k[0x8001] + 1 == k[0x8000] and k[0x0000] + 1 == k[0x0001]      # -denormal, -0.0, +0.0, +denormal


@pytest.mark.parametrize("name", ["uint8", "int8", "uint16", "int16"])
def test_keys_of_the_integers(name):
    info = np.iinfo(name)
    v = np.arange(info.min, info.max + 1).astype(name)
    k = R.key(v)
    assert k.dtype.kind == "u" and k.dtype.itemsize == v.dtype.itemsize
    assert np.array_equal(k.astype(np.int64), np.arange(len(v))) and np.array_equal(R.unkey(k, name), v)


# ---- the order of the contract on one small input -------------------------------------------------------------------------------------

def test_the_order_of_the_special_values():
    """seven samples in one window: the output at its centre, rank by rank, is the contract's order; NaNs of both signs and with
    payloads are one largest element and come out canonical; the zeros and the denormals keep their bits"""
    for bits in ([0xFFC00000, 0x7F800000, 0x80000000, 0x00000000, 0xFF800000, 0x00000001, 0x80000001],
                 [0x7F800001, 0xBF800000, 0xFFC12345, 0x007FFFFF, 0x807FFFFF, 0x7FC00000, 0x3F800000]):
        x = np.array(bits, dtype=np.uint32).view(np.float32).reshape(1, 1, 7)
        nan = [b for b in bits if (b & 0x7FFFFFFF) > 0x7F800000]
        rest = [b for b in bits if (b & 0x7FFFFFFF) <= 0x7F800000]
        want = sorted(rest, key=lambda b: (float(np.uint32(b).view(np.float32)), 0 if b >> 31 else 1)) + [0x7FC00000] * len(nan)
        got = [int(R.rank_filter(x, r, (1, 1, 7), mode="reflect").view(np.uint32)[0, 0, 3]) for r in range(7)]
        assert got == want, ([hex(g) for g in got], [hex(w) for w in want])
    zeros = np.array([0x80000000, 0x00000000], dtype=np.uint32).view(np.float32).reshape(1, 1, 2)
    assert R.rank_filter(zeros, 0, (1, 1, 2), origin=(0, 0, 0)).view(np.uint32)[0, 0, 0] == 0x80000000
    assert R.rank_filter(zeros, 1, (1, 1, 2), origin=(0, 0, 0)).view(np.uint32)[0, 0, 0] == 0x00000000


# ---- the restatement against scipy ----------------------------------------------------------------------------------------------------

BOXES = [(3, 3, 3), (1, 2, 5), (2, 3, 4), (7, 1, 3), (4, 4, 2), (5, 5, 5)]
SHAPES = [(5, 6, 9), (1, 1, 5), (2, 2, 2), (3, 1, 8)]      # (the small ones: a window wider than the axis, a reflection that wraps)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int16])
@pytest.mark.parametrize("box", BOXES)
def test_rank_filter_against_scipy(dtype, box):
    for shape, masked in itertools.product(SHAPES, (False, True)):
        A = tied(shape, 7, dtype)
        fp = random_mask(box, 3) if masked else None
        W = int(fp.sum()) if masked else int(np.prod(box))
        for mode, origin in itertools.product(R.MODES, ends_and_centre(box)):
            ordered = R.sorted_windows(A, box, fp, origin, mode, 2)
            for rank in sorted({0, 1 % W, W // 2, max(0, W - 2), W - 1}):
                want = ndi.rank_filter(A, rank, footprint=np.ones(box, dtype=bool) if fp is None else fp, mode=SCIPY_MODES[mode], cval=2,
                                       origin=scipy_origin(box, origin))
                got = R.pick(ordered, rank, A.dtype.name)
                assert got.dtype == A.dtype and np.array_equal(got, want), (shape, box, masked, mode, origin, rank)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8, np.int16])
def test_named_filters_against_scipy(dtype):
    A = tied((6, 7, 11), 9, dtype)
    for box, mode in itertools.product([(3, 3, 3), (2, 3, 4), (5, 1, 7)], R.MODES):
        for origin in ends_and_centre(box):
            kw = dict(size=box, mode=SCIPY_MODES[mode], cval=-1 if A.dtype.kind != "u" else 9, origin=scipy_origin(box, origin))
            ordered = R.sorted_windows(A, box, None, origin, mode, kw["cval"])
            W = len(ordered)
            assert np.array_equal(R.pick(ordered, W // 2, A.dtype.name), ndi.median_filter(A, **kw))
            assert np.array_equal(R.pick(ordered, 0, A.dtype.name), ndi.minimum_filter(A, **kw))
            assert np.array_equal(R.pick(ordered, W - 1, A.dtype.name), ndi.maximum_filter(A, **kw))
            for p in (0, 10, 37.5, 50, 99.9, 100, -25):
                q = p + 100.0 if p < 0 else p
                rank = W - 1 if q == 100 else int(float(W) * q / 100.0)
                assert np.array_equal(R.pick(ordered, rank, A.dtype.name), ndi.percentile_filter(A, p, **kw)), (box, mode, origin, p)
            assert np.array_equal(R.rank_filter(A, -2, box, None, origin, mode, kw["cval"]), ndi.rank_filter(A, -2, **kw))


def test_reflect_with_a_window_wider_than_the_axis():
    A = tied((2, 3, 1), 4, np.float32)
    for box in ((7, 7, 7), (5, 7, 3)):
        for origin in ends_and_centre(box):
            for rank in (0, 100, int(np.prod(box)) - 1):
                rank = min(rank, int(np.prod(box)) - 1)
                assert np.array_equal(R.rank_filter(A, rank, box, None, origin, "reflect"),
                                      ndi.rank_filter(A, rank, size=box, mode="reflect", origin=scipy_origin(box, origin)))


def test_one_and_two_dimensions_through_the_padding_rule():
    for dtype in (np.float32, np.uint8, np.int16):
        B = tied((9, 14), 5, dtype)
        for mode in R.MODES:
            for size, origin in (((3, 4), (0, 3)), ((5, 2), (2, 1))):
                got = R.rank_filter(R.pad3(B), 4, (1,) + size, None, (0,) + origin, mode, 1)[0]
                assert np.array_equal(got, ndi.rank_filter(B, 4, size=size, mode=mode, cval=1, origin=scipy_origin(size, origin)))
            fp = random_mask((3, 5), 8)
            got = R.rank_filter(R.pad3(B), 2, footprint=R.pad3(fp), mode=mode, cval=1)[0]
            assert np.array_equal(got, ndi.rank_filter(B, 2, footprint=fp, mode=mode, cval=1))
            for size, origin in ((5, 0), (4, 3), (7, 3)):
                got = R.rank_filter(R.pad3(B[3]), size // 2, (1, 1, size), None, (0, 0, origin), mode, 1)[0, 0]
                assert np.array_equal(got, ndi.rank_filter(B[3], size // 2, size=size, mode=mode, cval=1, origin=origin - size // 2))


# ---- the helpers of contourist_amd.volume ---------------------------------------------------------------------------------------------

def test_percentile_rank_is_scipys_rule():
    from contourist_amd import volume
    A = tied((4, 5, 9), 2, np.float32)
    for W, box in ((27, (3, 3, 3)), (24, (2, 3, 4)), (7, (7, 1, 1))):
        ordered = R.sorted_windows(A, box)
        assert len(ordered) == W
        for p in (0, 1, 10, 33.3, 50, 50.0, 75, 99, 99.99, 100, 100.0, -0.5, -25, -50, -100):
            rank = volume.percentile_rank(p, W)
            q = p + 100.0 if p < 0 else p
            assert rank == (W - 1 if q == 100 else int(float(W) * q / 100.0)) and 0 <= rank < W
            assert np.array_equal(R.pick(ordered, rank, "float32"), ndi.percentile_filter(A, p, size=box, mode="nearest"))
    for bad in (100.5, -100.5, 200):
        with pytest.raises(AssertionError):
            volume.percentile_rank(bad, 27)


def test_ball():
    from contourist_amd import volume
    assert volume.ball(0).shape == (1, 1, 1) and volume.ball(0.9).all()
    for r, connectivity in ((1, 1), (1.0, 1), (1.5, 2), (1.8, 3)):
        b = volume.ball(r)
        assert b.dtype == np.bool_ and np.array_equal(b, ndi.generate_binary_structure(3, connectivity))
    for r, side, count in ((2, 5, 33), (2.5, 5, 81), (3, 7, 123), (3.9, 7, 251)):
        b = volume.ball(r)
        d = np.arange(side) - side // 2
        want = d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2 <= r * r
        assert b.shape == (side,) * 3 and np.array_equal(b, want) and int(b.sum()) == count == int(want.sum())
        assert np.array_equal(b, b[::-1, ::-1, ::-1]) and np.array_equal(b, b.transpose(2, 0, 1))
    for bad in (4, 4.5, -1):
        with pytest.raises(AssertionError):
            volume.ball(bad)
