"""CPU: 3-D sample arrays of 8- and 16-bit types are kept in their type (the kernels read them as they are); the host-side
lookups see the same values as on the fp32 copy; the dtype codes of the C ABI; the library exports the typed entry points."""
import os
import re

import numpy as np
import pytest

from contourist_amd import _ffi, grid_field

HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "contourist_hip.h")
KEPT = (np.uint8, np.int8, np.uint16, np.int16, np.float16)


def _quantised(dtype, shape=(9, 8, 7), seed=3):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal(shape)
    if np.dtype(dtype).kind == "f":
        return (x * 10).astype(dtype)
    info = np.iinfo(dtype)
    lo, hi = max(info.min, -1000), min(info.max, 1000)
    return np.clip(np.rint(x * (hi - lo) / 8 + (lo + hi) / 2), lo, hi).astype(dtype)


@pytest.mark.parametrize("dtype", KEPT)
def test_from_array_keeps_3d_types(dtype):
    A = _quantised(dtype)
    g = grid_field.FunctionGrid.from_array(A)
    assert g.dense_samples().dtype == np.dtype(dtype)
    assert np.array_equal(g.dense_samples(), A)


@pytest.mark.parametrize("dtype", (np.float64, np.int32, np.int64))
def test_from_array_widens_inexact_types(dtype):
    A = _quantised(np.int16).astype(dtype)
    g = grid_field.FunctionGrid.from_array(A)
    assert g.dense_samples().dtype == np.float32
    assert np.array_equal(g.dense_samples(), A.astype(np.float32))


@pytest.mark.parametrize("shape", ((9, 8), (5, 6, 7, 4)))
def test_from_array_widens_2d_and_4d(shape):
    A = _quantised(np.int16, shape=shape)
    g = grid_field.FunctionGrid.from_array(A)
    assert g.dense_samples().dtype == np.float32
    assert np.array_equal(g.dense_samples(), A.astype(np.float32))


@pytest.mark.parametrize("dtype", KEPT)
def test_lookup_and_crossings_equal_the_widened_array(dtype):
    A = _quantised(dtype)
    g = grid_field.FunctionGrid.from_array(A, mins=[-1.0, 0.5, 2.0], delta=[0.5, 0.25, 1.0])
    w = grid_field.FunctionGrid.from_array(A.astype(np.float32), mins=[-1.0, 0.5, 2.0], delta=[0.5, 0.25, 1.0])
    for idx in ((0, 0, 0), (3, 4, 5), (8, 7, 6)):
        xyz = w.from_grid_coordinates(idx)
        assert g.f(*xyz) == w.f(*xyz) == float(A[idx])
    assert np.array_equal(g.dense_samples_host().astype(np.float64), w.dense_samples_host().astype(np.float64))
    value = float(np.median(A.astype(np.float64))) + 0.5 * (1 if np.dtype(dtype).kind != "f" else 0.01)
    for skip in (1, 2):
        a = g.find_contour_crossing_grid_segments(value, skip)
        b = w.find_contour_crossing_grid_segments(value, skip)
        assert a[0] == b[0] and a[1] == b[1]
        assert len(a[2]) == len(b[2]) > 0
        assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a[2], b[2]))


def test_dtype_codes():
    assert _ffi.DTYPE_CODES == {"float32": 0, "uint8": 1, "int8": 2, "uint16": 3, "int16": 4, "float16": 5, "bfloat16": 6}
    for name, code in _ffi.DTYPE_CODES.items():
        assert _ffi.dtype_code(name) == code
        if name != "bfloat16":
            assert _ffi.dtype_code(np.dtype(name)) == code
            assert _ffi.dtype_code(getattr(np, name)) == code
            assert _ffi.native_dtype(np.dtype(name))
    for bad in (np.float64, np.int32, np.int64, np.uint32, np.bool_, "complex64"):
        with pytest.raises(ValueError, match="not one the 3-D kernels read"):
            _ffi.dtype_code(bad)
        assert not _ffi.native_dtype(bad)


def test_torch_dtype_codes():
    torch = pytest.importorskip("torch")
    pairs = {torch.float32: 0, torch.uint8: 1, torch.int8: 2, torch.int16: 4, torch.float16: 5, torch.bfloat16: 6}
    if hasattr(torch, "uint16"):
        pairs[torch.uint16] = 3
    for t, code in pairs.items():
        assert _ffi.dtype_code(t) == code
    for bad in (torch.float64, torch.int32, torch.int64):
        with pytest.raises(ValueError):
            _ffi.dtype_code(bad)


def test_header_declares_the_typed_grid():
    text = open(HEADER).read()
    for name, code in _ffi.DTYPE_CODES.items():
        macro = "CX_DTYPE_" + {"float32": "F32", "uint8": "U8", "int8": "I8", "uint16": "U16", "int16": "I16",
                               "float16": "F16", "bfloat16": "BF16"}[name]
        assert re.search(r"#define %s %d\b" % (macro, code), text), macro
    for sym in ("cx_grid_upload_typed", "cx_grid_adopt_device_typed", "cx_grid_info"):
        assert re.search(r"\bint %s\(" % sym, text), sym
        assert sym in _ffi.SYMBOLS


def test_library_exports_typed_entry_points():
    from contourist_amd import build
    path = build.build()
    L = _ffi.load()
    for sym in ("cx_grid_upload_typed", "cx_grid_adopt_device_typed", "cx_grid_info"):
        assert hasattr(L, sym), sym
    assert os.path.exists(path)


@pytest.mark.parametrize("code", (">i2", ">u2", ">f2"))
def test_big_endian_arrays_are_read_by_value(code):
    """a big-endian 3-D array is kept in its type but in the machine's byte order (the kernels read raw bytes); the values and the
    host-side lookups are those of its fp32 copy"""
    A = _quantised(np.dtype(code).newbyteorder("="))
    big = A.astype(code)
    assert not big.dtype.isnative
    g = grid_field.FunctionGrid.from_array(big)
    d = g.dense_samples()
    assert d.dtype.isnative and d.dtype == A.dtype and np.array_equal(d, A)
    n = _ffi.native_array(big)
    assert n.dtype.isnative and n.flags.c_contiguous and np.array_equal(n, A)
    w = grid_field.FunctionGrid.from_array(big.astype(np.float32))
    assert g.f(1.0, 2.0, 3.0) == w.f(1.0, 2.0, 3.0) == float(A[1, 2, 3])
    value = float(np.median(A.astype(np.float64))) + 0.25
    a, b = g.find_contour_crossing_grid_segments(value), w.find_contour_crossing_grid_segments(value)
    assert len(a[2]) == len(b[2]) > 0 and all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a[2], b[2]))
