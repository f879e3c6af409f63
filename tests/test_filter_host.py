"""CPU: the numpy restatement of cx_grid_filter3d (tests/filter_ref.py) against scipy.ndimage, its stride and constant-field
properties, and the host side of contourist_amd.volume: the weight builders bit for bit and lattice_of."""
import numpy as np
import pytest

import filter_ref as R


def field(shape, seed):
    return (np.random.RandomState(seed).standard_normal(shape) * 3.0).astype(np.float32)


@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 4, 3), (9, 70, 131)])
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("sigma", [0.6, 1.0, 2.5])
def test_restatement_against_scipy(shape, mode, sigma):
    """within 2 ulp (fp32) of max|A|: three roundings of at most half an ulp each, plus the fp32 rounding of the weights (a relative
    2^-24 per weight, on a sum whose weights add up to 1)"""
    ndimage = pytest.importorskip("scipy.ndimage")
    A = field(shape, 7)
    want = ndimage.gaussian_filter(A.astype(np.float64), sigma, mode=mode, cval=1.5, truncate=4.0)
    got = R.gaussian(A, sigma, mode=mode, cval=1.5)
    ulp = float(np.spacing(np.float32(np.abs(A).max())))
    worst = float(np.abs(got.astype(np.float64) - want).max()) / ulp
    print("worst %.3f ulp of max|A|" % worst)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert worst <= 2.0


@pytest.mark.parametrize("mode", R.MODES)
def test_strided_result_is_the_unstrided_one_subsampled(mode):
    A = field((9, 10, 11), 3)
    full = R.gaussian(A, (1.0, 0.7, 1.4), mode=mode, cval=-2.0)
    part = R.gaussian(A, (1.0, 0.7, 1.4), stride=(2, 3, 2), mode=mode, cval=-2.0)
    assert part.shape == (5, 4, 6)
    assert np.array_equal(R.bits(part), R.bits(full[::2, ::3, ::2]))


def test_constant_field_stays_constant():
    A = np.full((6, 7, 20), 37, dtype=np.uint8)
    for mode in ("nearest", "reflect"):
        out = R.gaussian(A, 1.3, mode=mode)
        assert out.dtype == np.float32 and np.all(out == np.float32(37.0))
    assert np.all(R.pyramid(A, 3)[2] == np.float32(37.0)) and R.pyramid(A, 3)[2].shape == (2, 2, 5)


def test_unfiltered_axis_keeps_the_bits():
    A = field((3, 4, 5), 1)
    A[0, 0, 0], A[1, 1, 1] = -0.0, np.inf
    out = R.filter3d(A, [(None, 0, 2), (None, 0, 1), (None, 0, 3)])
    assert np.array_equal(R.bits(out), R.bits(A[::2, :, ::3]))


def test_lattice_of():
    from contourist_amd import volume
    mins, delta = volume.lattice_of((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), strides=(2, 1, 3), weights=R.gaussian_weights(1.0))
    assert np.array_equal(mins, [1.0, 2.0, 3.0]) and np.array_equal(delta, [1.0, 0.25, 6.0])
    # block_mean: origin 0, `factor` taps: the first output sits in the middle of the first block
    mins, delta = volume.lattice_of((1.0, 2.0, 3.0), 0.5, strides=(2, 3, 4), origins=0,
                                    weights=[volume.block_mean_weights(f) for f in (2, 3, 4)])
    assert np.array_equal(mins, [1.0 + 0.5 * 0.5, 2.0 + 1.0 * 0.5, 3.0 + 1.5 * 0.5]) and np.array_equal(delta, [1.0, 1.5, 2.0])
    # an axis that is not filtered does not move; an even kernel centred by default sits half a sample low
    mins, delta = volume.lattice_of((0.0, 0.0), (1.0, 1.0), weights=[None, np.ones(4, dtype=np.float32) / 4])
    assert np.array_equal(mins, [0.0, -0.5]) and np.array_equal(delta, [1.0, 1.0])
    mins, delta = volume.lattice_of((0.0,), 2.0, strides=2)
    assert np.array_equal(mins, [0.0]) and np.array_equal(delta, [4.0])


def test_weight_builders_bit_for_bit():
    from contourist_amd import volume
    for sigma in (0.3, 0.6, 1.0, 1.3, 2.5, 7.0, 16.0):
        for truncate in (4.0, 3.0):
            a, b = volume.gaussian_weights(sigma, truncate), R.gaussian_weights(sigma, truncate)
            assert a.dtype == np.float32 and len(a) == 2 * int(truncate * sigma + 0.5) + 1
            assert np.array_equal(R.bits(a), R.bits(b))
    assert volume.gaussian_weights(0.0) is None and R.gaussian_weights(0.0) is None
    for factor in (2, 3, 4, 7, 129):
        assert np.array_equal(R.bits(volume.block_mean_weights(factor)), R.bits(R.block_weights(factor)))
    assert volume.block_mean_weights(1) is None
    assert np.array_equal(R.bits(np.asarray(volume.PYRAMID_WEIGHTS, dtype=np.float32)), R.bits(R.PYRAMID.astype(np.float32)))
    assert volume.default_origin(5) == R.centre(5) == 2 and volume.default_origin(4) == R.centre(4) == 2


def test_locate_samples():
    "the four forms of `samples` every whole-volume operation of _ffi.Context takes -> (pointer, CX_DTYPE_* code, on_device, shape)"
    from contourist_amd import _ffi
    keep = []
    assert _ffi.locate_samples(None, keep) == (None, 0, 1, (0, 0, 0)) and keep == []
    # a numpy array: made contiguous, kept alive, its own type
    A = np.arange(4 * 5 * 6, dtype=np.int16).reshape(4, 5, 6)[:, :, ::2]
    assert not A.flags.c_contiguous
    ptr, code, on_device, shape = _ffi.locate_samples(A, keep)
    assert (code, on_device, shape) == (_ffi.DTYPE_CODES["int16"], 0, (4, 5, 3))
    assert len(keep) == 1 and keep[0].flags.c_contiguous and np.array_equal(keep[0], A) and ptr.value == keep[0].ctypes.data
    # a big-endian array is byte-swapped on the way
    ptr, code, on_device, shape = _ffi.locate_samples(np.arange(24, dtype=">u2").reshape(2, 3, 4), keep)
    assert (code, on_device, shape) == (_ffi.DTYPE_CODES["uint16"], 0, (2, 3, 4))
    assert len(keep) == 2 and keep[1].dtype.isnative and keep[1][1, 2, 3] == 23 and ptr.value == keep[1].ctypes.data
    # (device pointer, dtype, shape): nothing to keep
    ptr, code, on_device, shape = _ffi.locate_samples((0x7F0000001000, "uint8", [2, np.int64(3), 4]), keep)
    assert (ptr.value, code, on_device, shape) == (0x7F0000001000, 1, 1, (2, 3, 4)) and all(type(n) is int for n in shape) and len(keep) == 2
    # (numpy array, dtype, shape): host bytes of a type numpy has no name for
    B = np.zeros((2, 3, 8), dtype=np.uint16)
    ptr, code, on_device, shape = _ffi.locate_samples((B, "bfloat16", (2, 3, 8)), keep)
    assert (ptr.value, code, on_device, shape) == (B.ctypes.data, 6, 0, (2, 3, 8)) and keep[2] is B
    ptr, code, on_device, shape = _ffi.locate_samples((B[:, :, ::2], "bfloat16", (2, 3, 4)), keep)
    assert (code, on_device, shape) == (6, 0, (2, 3, 4)) and keep[3].flags.c_contiguous and ptr.value == keep[3].ctypes.data != B.ctypes.data
    with pytest.raises(ValueError):
        _ffi.locate_samples(np.zeros((2, 2, 2), dtype=np.float64), keep)
    with pytest.raises(AssertionError):
        _ffi.locate_samples(np.zeros((2, 2), dtype=np.float32), keep)
