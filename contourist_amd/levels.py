"""Choosing isovalues on the device: exact order statistics of a sample array (`cx_samples_select`) and the size of the
isosurface at every one of many candidate values (`cx_level_spectrum3d`), csrc/cx_pick.hip.

The rules of the reference's level pickers (contourist/multiple_2d_contour.py:84-108: Percentile2DContour sorts all lattice
samples and takes every (N / breakpoints)-th, Linear2DContour takes multiples of (max - min) / breakpoints) are restated here on
ranks, so the sort never happens: `percentile_values` and `linear_values` return the same float64 values bit for bit.

Samples are a numpy array or a tensor already on the GPU, of any number of dimensions.  Types the kernels read (float32, uint8,
int8, uint16, int16, float16, bfloat16) are used as they are; any other type is converted to float32 first, and the order is that
of the float32 values (numpy's: -inf < finite < +inf < NaN).
"""
import numpy as np

from . import _ffi
from . import grid_field

MAX_RANKS = 1024      # per call of cx_samples_select
MAX_LEVELS = 4096     # per call of cx_level_spectrum3d

_contexts = {}


def _context(device=None):
    "one context per device for the calls of this module (its scratch is kept between calls)"
    if device is None:
        from . import triangulated
        device = triangulated._DEFAULT_DEVICE[0]
    device = int(device)
    if device not in _contexts:
        _contexts[device] = _ffi.Context(device)
    return _contexts[device]


def _prepared(samples):
    "(samples in a type the kernels read, contiguous; True if it is a device tensor)"
    if grid_field._is_torch(samples):
        t = samples
        if not _ffi.native_dtype(t.dtype):
            t = t.float()
        assert t.is_cuda, "a tensor of samples must be on the GPU (pass host samples as a numpy array)"
        return t.contiguous(), True
    a = np.asarray(samples)
    if not _ffi.native_dtype(a.dtype):
        a = a.astype(np.float32)
    return _ffi.native_array(a), False


def _size(samples):
    return int(samples.numel()) if grid_field._is_torch(samples) else int(np.asarray(samples).size)


def order_statistics(samples, ranks, device=None, context=None):
    """-> (values float64 in the order of `ranks`, number of NaN samples): values[k] is
    np.sort(samples.astype(np.float32), axis=None)[ranks[k]], exactly.  Any number of ranks (1024 go into one call)."""
    s, on_device = _prepared(samples)
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    assert len(ranks) >= 1, "at least one rank"
    if context is None:
        context = _context(s.device.index if on_device and device is None else device)
    values, n_nan = [], 0
    for first in range(0, len(ranks), MAX_RANKS):
        chunk = ranks[first:first + MAX_RANKS]
        if on_device:
            v, n_nan = context.samples_select(chunk, int(s.data_ptr()), dtype=s.dtype, n=int(s.numel()))
        else:
            v, n_nan = context.samples_select(chunk, s)
        values.append(v)
    return np.concatenate(values), n_nan


def quantile_ranks(q, n_valid):
    "rank floor(q (n_valid - 1)) of every q in [0, 1], in float64: np.nanquantile(..., method='lower')"
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    assert n_valid >= 1, "no sample that is not NaN"
    assert np.all((q >= 0.0) & (q <= 1.0)), "quantiles lie in [0, 1]"
    return np.floor(q * np.float64(n_valid - 1)).astype(np.int64)


def quantiles(samples, q, device=None):
    "the q-quantiles (q in [0, 1], scalar or sequence) over the samples that are not NaN -> float64 array"
    s, _ = _prepared(samples)
    _, n_nan = order_statistics(s, [0], device)
    values, _ = order_statistics(s, quantile_ranks(q, _size(s) - n_nan), device)
    return values


def percentile_ranks(size, breakpoints):
    "the ranks behind ordered[stride::stride], stride = int(size / breakpoints) (multiple_2d_contour.py:84-98)"
    stride = int(size / breakpoints)
    return np.arange(size, dtype=np.int64)[stride::stride]


def percentile_values(samples, breakpoints, device=None):
    "Percentile2DContour's levels: every (N / breakpoints)-th of the sorted samples, as a list of float64"
    ranks = percentile_ranks(_size(samples), breakpoints)
    if len(ranks) == 0:
        return []
    return list(order_statistics(samples, ranks, device)[0])


def linear_values(samples, breakpoints, device=None):
    "Linear2DContour's levels: the multiples 1 .. breakpoints - 1 of (max - min) * (1 / breakpoints), as a list of float64"
    (low, high), _ = order_statistics(samples, [0, _size(samples) - 1], device)
    step = (high - low) * (1.0 / breakpoints)
    return [step * k for k in range(1, breakpoints)]


def spectrum_of_context(context, values):
    "cx_level_spectrum3d on the grid bound to `context`, any number of values (4096 go into one call) -> dict of int64 arrays"
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    parts = [context.level_spectrum3d(values[first:first + MAX_LEVELS]) for first in range(0, len(values), MAX_LEVELS)]
    return {k: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dtype=np.int64) for k in _ffi.SPECTRUM_KEYS}


def spectrum(samples, values, device=None):
    """the size of the isosurface of a 3-D sample array at every one of `values`, without marching any -> dict of four int64 arrays
    in the order of `values`: n_cells (whole lattice cells the surface passes through), n_vertices, n_triangles -- what an
    extraction at that value returns as n_border_voxels, n_vertices and n_triangles wherever n_near is 0 -- and n_near (samples
    inside the march's tolerance screen of that value)"""
    s, on_device = _prepared(samples)
    assert len(s.shape) == 3, "3-D sample array expected"
    context = _context(s.device.index if on_device and device is None else device)
    if on_device:
        context.adopt_device_grid(s.data_ptr(), tuple(int(n) for n in s.shape), keepalive=s, dtype=s.dtype)
    else:
        context.upload_grid_native(s)
    return spectrum_of_context(context, values)
