"""Preparing the volume on the device: smoothing, binning and level-of-detail pyramids of a sample array before it is marched
(`cx_grid_filter3d`, csrc/cx_filter.hip).

Everything here is one operation: per axis a row of fp32 weights, an origin and a stride,

    out[i] = (float32) sum_k float64(weights[k]) * float64(in[src(i * stride + k - origin)])

summed in float64 with k ascending and rounded to float32 once per axis; the axes are filtered last axis first, float32 between
them.  `src` is the boundary rule: "nearest", "reflect" or "constant" (`cval`), as scipy.ndimage names them.  tests/filter_ref.py
restates it in numpy and the device result equals it bit for bit.

Samples are a numpy array or a contiguous tensor already on the GPU, of 1 to 3 dimensions (missing leading axes count as axes of
length 1 that are not filtered).  Types the kernels read (float32, uint8, int8, uint16, int16, float16, bfloat16) are loaded as
they are and converted in registers; any other type is converted to float32 first.  The result is float32: a numpy array for numpy
samples, a device tensor for a tensor.

`lattice_of` gives the `(mins, delta)` of the result's lattice, so that a result goes straight into
`FunctionGrid.from_array(result, mins, delta)` or `MultiLevelIsosurfaces` and lands where the data is.
"""
import numpy as np

from . import _ffi
from . import grid_field

MAX_WEIGHTS = 129      # per axis of cx_grid_filter3d
PYRAMID_WEIGHTS = (1.0 / 16.0, 4.0 / 16.0, 6.0 / 16.0, 4.0 / 16.0, 1.0 / 16.0)

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


def _per_axis(value, ndim, neutral, name):
    "a scalar for all axes of the array, or one value per axis of the array -> three values, `neutral` on the padded leading axes"
    if np.ndim(value) == 0:
        vals = [value] * ndim
    else:
        vals = list(value)
        assert len(vals) == ndim, "%s: one value or one per axis of the samples (%d)" % (name, ndim)
    return [neutral] * (3 - ndim) + vals


def _weights_per_axis(weights, ndim):
    "one 1-D row of weights for all axes of the array, or a list with a row or None per axis -> three rows (float32) or None"
    per_axis = isinstance(weights, (list, tuple)) and len(weights) == ndim and all(w is None or np.ndim(w) == 1 for w in weights)
    rows = list(weights) if per_axis else [weights] * ndim
    out = [None] * (3 - ndim)
    for w in rows:
        if w is None:
            out.append(None)
            continue
        w = np.ascontiguousarray(w, dtype=np.float32)
        assert w.ndim == 1 and 1 <= len(w) <= MAX_WEIGHTS, "1 to %d weights per axis" % MAX_WEIGHTS
        out.append(w)
    return out


def default_origin(n_weights):
    "the tap that sits on the output sample when no origin is given: the middle one, n_weights // 2 (scipy.ndimage's centre)"
    return int(n_weights) // 2


def gaussian_weights(sigma, truncate=4.0):
    """scipy.ndimage's Gaussian kernel: exp(-k^2 / (2 sigma^2)) for k = -r .. r, r = int(truncate * sigma + 0.5), computed and
    normalised in float64, then rounded to float32.  None for sigma == 0 (the axis is not filtered)."""
    sigma = float(sigma)
    assert sigma >= 0.0 and np.isfinite(sigma), "sigma is a finite number >= 0"
    if sigma == 0.0:
        return None
    radius = int(float(truncate) * sigma + 0.5)
    assert 2 * radius + 1 <= MAX_WEIGHTS, "truncate * sigma is at most %d samples" % ((MAX_WEIGHTS - 1) // 2)
    k = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    return (phi / phi.sum()).astype(np.float32)


def block_mean_weights(factor):
    "`factor` taps of 1 / factor (the float32 nearest to it); None for factor 1"
    factor = int(factor)
    assert 1 <= factor <= MAX_WEIGHTS, "a factor of 1 to %d" % MAX_WEIGHTS
    if factor == 1:
        return None
    return np.full(factor, np.float64(1.0) / np.float64(factor)).astype(np.float32)


def convolve_separable(samples, weights, strides=1, origins=None, mode="nearest", cval=0.0, device=None):
    """the operation of this module.  weights: one 1-D row for all axes, or a list with one row or None (axis not filtered) per axis
    of `samples`; strides, origins: one value or one per axis; origins None: the middle tap (`default_origin`).  An axis keeps every
    stride-th output: ceil(n / stride) samples."""
    on_device = grid_field._is_torch(samples)
    if on_device:
        t = samples
        assert t.is_cuda, "a tensor of samples must be on the GPU (pass host samples as a numpy array)"
        if not _ffi.native_dtype(t.dtype):
            t = t.float()
        assert t.is_contiguous(), "a tensor of samples must be contiguous"
        shape = tuple(int(n) for n in t.shape)
    else:
        a = np.asarray(samples)
        if not _ffi.native_dtype(a.dtype):
            a = a.astype(np.float32)
        a = _ffi.native_array(a)
        shape = tuple(int(n) for n in a.shape)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    rows = _weights_per_axis(weights, ndim)
    st = [int(s) for s in _per_axis(strides, ndim, 1, "strides")]
    if origins is None:
        og = [0 if w is None else default_origin(len(w)) for w in rows]
    else:
        og = [int(o) for o in _per_axis(origins, ndim, 0, "origins")]
    axes = [(rows[k], og[k] if rows[k] is not None else 0, st[k]) for k in range(3)]
    shape3 = (1,) * (3 - ndim) + shape
    if on_device:
        import torch
        context = _context(t.device.index if device is None else device)
        out = torch.empty([-(-shape3[k] // max(1, st[k])) for k in range(3)], dtype=torch.float32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()      # the samples are there; the context has a stream of its own
        got, _ = context.filter_grid(axes, mode, cval, samples=(t.data_ptr(), t.dtype, shape3), out=out.data_ptr())
        context.synchronize()
        assert got == tuple(out.shape)
        return out.reshape(got[3 - ndim:])
    context = _context(device)
    got, result = context.filter_grid(axes, mode, cval, samples=a.reshape(shape3), download=True)
    return result.reshape(got[3 - ndim:])


def gaussian(samples, sigma, truncate=4.0, stride=1, mode="nearest", cval=0.0, device=None):
    """scipy.ndimage.gaussian_filter of the float32 samples, every stride-th sample kept.  sigma, stride: one value or one per axis;
    sigma == 0 leaves an axis unfiltered."""
    ndim = len(samples.shape)
    sig = _per_axis(sigma, ndim, 0.0, "sigma")[3 - ndim:]
    return convolve_separable(samples, [gaussian_weights(s, truncate) for s in sig], stride, None, mode, cval, device)


def block_mean(samples, factor, mode="nearest", cval=0.0, device=None):
    """the mean over blocks of `factor` samples (one value or one per axis): `factor` taps of 1 / factor from the block's first sample,
    stride `factor`.  A partial last block is completed by the boundary rule."""
    ndim = len(samples.shape)
    fac = [int(f) for f in _per_axis(factor, ndim, 1, "factor")[3 - ndim:]]
    return convolve_separable(samples, [block_mean_weights(f) for f in fac], fac, 0, mode, cval, device)


def pyramid(samples, levels, mode="nearest", cval=0.0, device=None):
    "[samples, half, quarter, ...] (`levels` arrays): each the one before filtered with [1, 4, 6, 4, 1] / 16 at stride 2"
    out = [samples]
    for _ in range(int(levels) - 1):
        prev = out[-1]
        strides = [2 if int(n) >= 2 else 1 for n in prev.shape]
        rows = [np.asarray(PYRAMID_WEIGHTS, dtype=np.float32) if int(n) >= 2 else None for n in prev.shape]
        out.append(convolve_separable(prev, rows, strides, None, mode, cval, device))
    return out


def lattice_of(mins, delta, strides=1, origins=None, weights=None):
    """(mins, delta) of the lattice of a result, given those of the samples: delta times the stride, mins shifted by
    (n_weights - 1) / 2 - origin samples -- the centre of the taps of output 0.  Zero for a centred kernel of odd length,
    (factor - 1) / 2 for `block_mean`.  weights: as in `convolve_separable`; None: nothing is shifted."""
    mins = np.asarray(mins, dtype=np.float64).reshape(-1)
    ndim = len(mins)
    delta = np.asarray(_per_axis(delta, ndim, 1.0, "delta")[3 - ndim:] if np.ndim(delta) else [delta] * ndim, dtype=np.float64)
    st = np.asarray(_per_axis(strides, ndim, 1, "strides")[3 - ndim:], dtype=np.float64)
    if weights is None:
        taps = [0] * ndim
    else:
        taps = [0 if w is None else len(w) for w in _weights_per_axis(weights, ndim)[3 - ndim:]]
    if origins is None:
        og = [default_origin(n) for n in taps]
    else:
        og = [int(o) for o in _per_axis(origins, ndim, 0, "origins")[3 - ndim:]]
    shift = np.asarray([(n - 1) / 2.0 - o if n else 0.0 for n, o in zip(taps, og)], dtype=np.float64)
    return mins + shift * delta, delta * st


# ---- distance fields (cx_grid_distance3d, csrc/cx_dist.hip) ---------------------------------------------------------------------------
# A sample f is LOW iff float64(f) < value (a NaN is never low): the march's own classification.  The squared distance is a minimum per
# axis, last axis first, in float64 (include/contourist_hip.h, "distance fields"; tests/distance_ref.py restates it and the device result
# equals it bit for bit).  With unit sampling it is the exact squared Euclidean distance.

def _distance_samples(samples):
    "-> (on_device, the samples in a type the kernels read, their shape)"
    if grid_field._is_torch(samples):
        import torch
        t = samples
        assert t.is_cuda, "a tensor of samples must be on the GPU (pass host samples as a numpy array)"
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        elif not _ffi.native_dtype(t.dtype):
            t = t.float()
        assert t.is_contiguous(), "a tensor of samples must be contiguous"
        return True, t, tuple(int(n) for n in t.shape)
    a = np.asarray(samples)
    if a.dtype == np.bool_:
        a = a.view(np.uint8)
    elif not _ffi.native_dtype(a.dtype):
        a = a.astype(np.float32)
    a = _ffi.native_array(a)
    return False, a, tuple(int(n) for n in a.shape)


def _distance_steps(steps, device, samples):
    """runs the transforms `steps` = [(value, side, kind, radius2), ...], each on the result of the one before (which stays on the
    device), on `samples` -> the last result: a numpy array for numpy samples, a device tensor for a tensor"""
    on_device, s, shape = samples
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    shape3 = (1,) * (3 - ndim) + shape
    sampling = steps[0][4]
    if sampling is not None:
        sampling = [float(x) for x in _per_axis(sampling, ndim, 1.0, "sampling")]
    if on_device:
        import torch
        torch_types = {"squared": torch.float64, "float32": torch.float32, "mask": torch.uint8}
        context = _context(s.device.index if device is None else device)
        torch.cuda.current_stream(s.device).synchronize()      # the samples are there; the context has a stream of its own
        src, result = (s.data_ptr(), s.dtype, shape3), None
        for value, side, kind, radius2, _ in steps:
            out = torch.empty(shape3, dtype=torch_types[kind], device=s.device)
            context.distance_grid(value, side, kind, sampling, radius2, samples=src, out=out.data_ptr())
            src, result = (out.data_ptr(), out.dtype, shape3), out
        return result.reshape(shape)
    context = _context(device)
    src = s.reshape(shape3)
    for n, (value, side, kind, radius2, _) in enumerate(steps):
        if n + 1 < len(steps):      # stays in the context; the next step reads it there
            _, ptr = context.distance_grid(value, side, kind, sampling, radius2, samples=src)
            src = (ptr, "uint8", shape3)
        else:
            _, result = context.distance_grid(value, side, kind, sampling, radius2, samples=src, download=True)
    return result.reshape(shape)


def distance(samples, value, side="below", sampling=None, squared=False, device=None):
    """the Euclidean distance from every sample to the nearest site, float32 (squared=True: the squared distance, float64).
    side "below": the sites are the samples with f >= value, the result is 0 there and positive where f < value
    (scipy.ndimage.distance_transform_edt(f < value)); "above": the sites are the samples with f < value (edt(f >= value)); "signed":
    above minus below, which has the sign of f - value.  Without a site the result is +inf.
    sampling: None (1 per axis), one step or one per axis of the samples; `sampling=delta` gives world units.  The result lives on
    the samples' own lattice: the same (mins, delta), `lattice_of(mins, delta)` with no weights.
    Samples: a numpy array (a numpy array comes back) or a contiguous GPU tensor (a tensor comes back) of 1 to 3 dimensions."""
    return _distance_steps([(value, side, "squared" if squared else "float32", 0.0, sampling)], device, _distance_samples(samples))


def signed_distance(samples, value, sampling=None, device=None):
    """distance(..., side="signed"): negative where f < value, positive where f >= value, never 0.  Marching it at 0 gives the surface
    of f at `value` without the staircase of a mask, wound the same way; marching it at d gives the offset surface at distance d.
    `sampling=delta` gives world units; the result's lattice is the samples' (`lattice_of(mins, delta)` with no weights)."""
    return distance(samples, value, "signed", sampling, False, device)


def _radius2(radius):
    radius = float(radius)
    assert radius >= 0.0 and np.isfinite(radius), "radius is a finite number >= 0"
    return radius * radius


def _inverted(mask):
    return mask.bitwise_xor_(1) if grid_field._is_torch(mask) else mask ^ np.uint8(1)


def dilate(samples, value, radius, sampling=None, device=None):
    """the set {f >= value} grown by a ball: uint8, 1 where a sample of the set lies within `radius` (squared distance <= radius^2).
    `sampling=delta` gives the radius world units; the mask's lattice is the samples' (`lattice_of(mins, delta)` with no weights)."""
    return _distance_steps([(value, "below", "mask", _radius2(radius), sampling)], device, _distance_samples(samples))


def erode(samples, value, radius, sampling=None, device=None):
    """the set {f >= value} shrunk by a ball: uint8, 1 where no sample outside the set lies within `radius`.  The array's rim does not
    erode: there is nothing outside the array.  Sampling and lattice as in `dilate`."""
    return _inverted(_distance_steps([(value, "above", "mask", _radius2(radius), sampling)], device, _distance_samples(samples)))


def opened(samples, value, radius, sampling=None, device=None):
    """erode, then dilate: removes what a ball of `radius` does not fit into (specks, thin bridges).  The second transform runs on the
    first one's mask where it lies on the device, thresholded at 0.5.  Sampling and lattice as in `dilate`."""
    r2 = _radius2(radius)
    # the first mask is 1 where the set is eroded away: the eroded set is its zeros, the sites of "above" at 0.5
    return _distance_steps([(value, "above", "mask", r2, sampling), (0.5, "above", "mask", r2, sampling)], device, _distance_samples(samples))


def closed(samples, value, radius, sampling=None, device=None):
    """dilate, then erode: fills what a ball of `radius` does not fit into (pinholes, thin gaps).  The second transform runs on the
    first one's mask where it lies on the device, thresholded at 0.5.  Sampling and lattice as in `dilate`."""
    r2 = _radius2(radius)
    return _inverted(_distance_steps([(value, "below", "mask", r2, sampling), (0.5, "above", "mask", r2, sampling)], device, _distance_samples(samples)))



# ---- connected components (cx_grid_label3d, csrc/cx_label.hip) -----------------------------------------------------------------------
# The objects of the thresholded volume: labels numbered by the linear index of each component's first sample (scipy.ndimage.label's
# own numbering), one record of exact integers per component, and masks chosen by label.  tests/label_ref.py restates it in numpy and
# the device result equals it exactly.  A result's lattice is the samples' own: the same (mins, delta), `lattice_of(mins, delta)` with
# no weights.

def _label_samples(samples):
    "-> (on_device, the samples in a type the kernels read, their shape, the shape padded to three axes, the argument of label_grid)"
    on_device, s, shape = _distance_samples(samples)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    shape3 = (1,) * (3 - ndim) + shape
    if on_device:
        import torch
        torch.cuda.current_stream(s.device).synchronize()      # the samples are there; the context has a stream of its own
        return True, s, shape, shape3, (s.data_ptr(), s.dtype, shape3)
    return False, s, shape, shape3, s.reshape(shape3)


def _device_view(ptr, shape, typestr, device):
    "a tensor over device memory of the context's (no copy): valid as long as that buffer is"
    import torch

    class _View(object):
        def __init__(self):
            self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(_View(), device=device)


def label(samples, value, side="high", connectivity=1, measures=False, device=None):
    """scipy.ndimage.label of the thresholded samples -> (labels int32, K), with measures=True (labels, K, records).
    side "high": the samples with f >= value (and the NaNs) are labelled; "low": those with f < value.  connectivity 1, 2, 3: 6, 18 or
    26 neighbours in three dimensions (offsets that differ on at most `connectivity` axes).  Labels are 1..K in the order of each
    component's first sample in C order, 0 elsewhere.  records: one `_ffi.LABEL_COMPONENT_DTYPE` per component, record c - 1 for label
    c: voxels, first, sum, lo, hi, rim over the three axes of the padded shape (missing leading axes have length 1).
    Samples: a numpy array (a numpy array comes back) or a contiguous GPU tensor (a tensor comes back) of 1 to 3 dimensions; bool
    samples count as 0 and 1."""
    on_device, s, shape, shape3, arg = _label_samples(samples)
    if not on_device:
        context = _context(device)
        k, labels = context.label_grid(value, side, connectivity, samples=arg, download=True)
        labels = labels.reshape(shape)
    else:
        import torch
        context = _context(s.device.index if device is None else device)
        if measures:      # the records describe labels the context holds: those are copied once on the device
            k, ptr = context.label_grid(value, side, connectivity, samples=arg)
            labels = _device_view(ptr, shape, "<i4", s.device).clone()
            torch.cuda.current_stream(s.device).synchronize()      # (the context's buffer is free for its next call)
        else:
            labels = torch.empty(shape3, dtype=torch.int32, device=s.device)
            k, _ = context.label_grid(value, side, connectivity, samples=arg, out=labels.data_ptr())
            labels = labels.reshape(shape)
    return (labels, k, context.label_measures()) if measures else (labels, k)


def _selected(context, on_device, s, shape, shape3, keep):
    "the mask of the labels the context holds: a tensor beside the samples `s`, or a numpy array"
    if on_device:
        import torch
        out = torch.empty(shape3, dtype=torch.uint8, device=s.device)
        context.label_select(keep, out=out.data_ptr())
        return out.reshape(shape)
    return context.label_select(keep, download=True)[1].reshape(shape)


def keep_components(samples, value, side="high", connectivity=1, largest=None, min_voxels=None, rim=None, keep=None, device=None):
    """uint8 mask of the components of `label(samples, value, side, connectivity)` that pass every criterion given:
    min_voxels=n: at least n voxels; rim=True / False: only components that touch / do not touch the array's rim (on an axis of the
    samples; padded leading axes do not count); keep: a bool array over the labels 1..K, or a callable that gets the records and
    returns one; largest=k, applied last: of what is left, the k components with the most voxels, ties going to the smaller label.
    The criteria are evaluated on the host from the records (K of them); the labels and the mask never leave the device for a tensor."""
    on_device, s, shape, shape3, arg = _label_samples(samples)
    context = _context((s.device.index if on_device else None) if device is None else device)
    k, _ = context.label_grid(value, side, connectivity, samples=arg)
    records = context.label_measures()
    ok = np.ones(k, dtype=bool)
    if min_voxels is not None:
        ok &= records["voxels"] >= int(min_voxels)
    if rim is not None:
        real = 0
        for axis in range(3 - len(shape), 3):
            real |= 3 << (2 * axis)
        touches = (records["rim"] & np.uint32(real)) != 0
        ok &= touches if rim else ~touches
    if keep is not None:
        flags = np.asarray(keep(records) if callable(keep) else keep).astype(bool).reshape(-1)
        assert len(flags) == k, "keep: one flag per component (%d)" % k
        ok &= flags
    if largest is not None:
        cand = np.flatnonzero(ok)
        order = cand[np.argsort(-records["voxels"][cand], kind="stable")]      # stable: the smaller label first among equals
        ok = np.zeros(k, dtype=bool)
        ok[order[:max(0, int(largest))]] = True
    return _selected(context, on_device, s, shape, shape3, np.concatenate([[False], ok]))


def remove_small(samples, value, min_voxels, connectivity=1, device=None):
    "the set {f >= value} without its components of fewer than `min_voxels` voxels: uint8"
    return keep_components(samples, value, "high", connectivity, min_voxels=min_voxels, device=device)


def clear_border(samples, value, connectivity=1, device=None):
    "the set {f >= value} without the components that touch the array's rim (skimage.segmentation.clear_border): uint8"
    return keep_components(samples, value, "high", connectivity, rim=False, device=device)


def fill_holes(samples, value, connectivity=1, device=None):
    """the set {f >= value} united with the components of {f < value}, labelled with `connectivity`, that do not touch the array's rim:
    uint8.  scipy.ndimage.binary_fill_holes(f >= value, generate_binary_structure(3, connectivity))."""
    on_device, s, shape, shape3, arg = _label_samples(samples)
    context = _context((s.device.index if on_device else None) if device is None else device)
    k, _ = context.label_grid(value, "low", connectivity, samples=arg)
    records = context.label_measures()
    real = 0
    for axis in range(3 - len(shape), 3):
        real |= 3 << (2 * axis)
    enclosed = (records["rim"] & np.uint32(real)) == 0
    return _selected(context, on_device, s, shape, shape3, np.concatenate([[True], enclosed]))


# ---- resampling through an affine map (cx_grid_resample3d, csrc/cx_resample.hip) ------------------------------------------------------
# out[i] = f(offset + matrix @ i): the matrix maps the OUTPUT index to the INPUT index, scipy.ndimage.affine_transform's convention,
# computed in float64 with every product and sum rounded on its own.  order 0 reads the nearest sample, floor(c + 0.5), in the samples'
# own type; order 1 blends the eight corners around floor(c) in float64 (input axis 2 first, then 1, then 0) and rounds to float32 once.
# Modes "nearest", "reflect" and "constant" are scipy's 'nearest', 'reflect' and 'grid-constant'.  tests/resample_ref.py restates it in
# numpy and the device result equals it bit for bit.

def _map3(matrix, offset, ndim):
    "(matrix, offset) of an array of `ndim` axes -> the 3 x 3 matrix and 3-vector of the array padded with leading axes of length 1"
    M = np.asarray(matrix, dtype=np.float64)
    if M.ndim == 0:
        M = np.full(ndim, float(M))
    if M.ndim == 1:
        assert len(M) in (ndim, 3), "matrix: a vector of one factor per axis of the samples (%d)" % ndim
        M = np.diag(M)
    assert M.shape in ((ndim, ndim), (3, 3)), "matrix: %d x %d or 3 x 3" % (ndim, ndim)
    off = np.asarray(offset, dtype=np.float64)
    if off.ndim == 0:
        off = np.full(M.shape[0], float(off))
    off = off.reshape(-1)
    assert len(off) == M.shape[0], "offset: one value or one per row of the matrix"
    M3, off3 = np.eye(3), np.zeros(3)
    k = 3 - M.shape[0]
    M3[k:, k:] = M
    off3[k:] = off
    return M3, off3


def resample(samples, matrix, offset=0, output_shape=None, order=1, mode="nearest", cval=0.0, device=None, return_outside=False):
    """scipy.ndimage.affine_transform(samples, matrix, offset, output_shape, order=order) for order 0 and 1.
    matrix: 3 x 3 (ndim x ndim for samples of fewer dimensions), or a vector, which means a diagonal; offset: one value or one per
    axis; output_shape None: the samples' shape.  order 0 returns the samples' own type, order 1 float32.
    return_outside=True: (result, n_outside), the number of output samples whose source coordinate lies off the array on some axis.
    Samples: a numpy array (a numpy array comes back) or a contiguous GPU tensor (a tensor comes back) of 1 to 3 dimensions."""
    on_device, s, shape = _distance_samples(samples)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    assert int(order) in (0, 1), "order 0 or 1"
    M3, off3 = _map3(matrix, offset, ndim)
    out_shape = shape if output_shape is None else tuple(int(n) for n in output_shape)
    assert len(out_shape) == ndim, "output_shape: one length per axis of the samples (%d)" % ndim
    shape3, out3 = (1,) * (3 - ndim) + shape, (1,) * (3 - ndim) + out_shape
    if on_device:
        import torch
        context = _context(s.device.index if device is None else device)
        out = torch.empty(out3, dtype=s.dtype if int(order) == 0 else torch.float32, device=s.device)
        torch.cuda.current_stream(s.device).synchronize()      # the samples are there; the context has a stream of its own
        n_outside, _ = context.resample_grid(M3, off3, out3, order, mode, cval, samples=(s.data_ptr(), s.dtype, shape3), out=out.data_ptr())
        result = out.reshape(out_shape)
    else:
        context = _context(device)
        n_outside, result = context.resample_grid(M3, off3, out3, order, mode, cval, samples=s.reshape(shape3), download=True)
        result = result.reshape(out_shape)
    return (result, n_outside) if return_outside else result


def _corner_scale(n, m):
    """the step d of `zoom`'s "corners": (n - 1) / (m - 1), moved by a few units in its last place where that makes the last
    coordinate (m - 1) d, rounded as the kernel rounds it, exactly n - 1; where no such neighbour exists, the nearest step that does not
    fall short of n - 1 (the last output then reads the last sample under "nearest" and "reflect", and counts as outside)"""
    if m <= 1 or n <= 1:
        return 0.0
    last, steps = np.float64(n - 1), np.float64(m - 1)
    d = last / steps
    lo = hi = d
    near = [d]
    for _ in range(4):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        near += [lo, hi]
    for x in near:
        if steps * x == last:
            return float(x)
    while steps * d < last:
        d = np.nextafter(d, np.inf)
    return float(d)


def zoom_map(shape, factor, align="centers"):
    "(matrix diagonal, offset, output shape) of `zoom` for samples of `shape`"
    ndim = len(shape)
    fac = [float(f) for f in _per_axis(factor, ndim, 1.0, "factor")[3 - ndim:]]
    assert all(f > 0.0 and np.isfinite(f) for f in fac), "factor is a finite number > 0"
    out = tuple(max(1, int(round(int(n) * f))) for n, f in zip(shape, fac))
    if align == "centers":
        diag = np.asarray([1.0 / f for f in fac], dtype=np.float64)
        return diag, 0.5 * diag - 0.5, out
    assert align == "corners", "align: 'centers' or 'corners'"
    return np.asarray([_corner_scale(int(n), m) for n, m in zip(shape, out)], dtype=np.float64), np.zeros(ndim), out


def zoom(samples, factor, order=1, mode="nearest", align="centers", cval=0.0, device=None):
    """the samples at `factor` times the resolution (one factor or one per axis): round(n * factor) samples per axis, at least 1.
    align "centers": samples are cell centres and the array keeps its extent, c = (i + 0.5) / factor - 0.5 -- what
    scipy.ndimage.zoom(samples, factor, order=order, mode=..., grid_mode=True) reads wherever n * factor is an integer (scipy divides
    by the ratio of the lengths, which is the factor then), with scipy's mode 'grid-constant' for "constant".
    align "corners": the first and last sample keep their place, c = i (n - 1) / (m - 1) -- scipy.ndimage.zoom's default
    (grid_mode=False), the step adjusted in its last place so that the last output lands on the last sample (`_corner_scale`): the
    corner samples are reproduced exactly under "nearest" and "reflect"."""
    shape = tuple(int(n) for n in samples.shape)
    diag, off, out = zoom_map(shape, factor, align)
    return resample(samples, diag, off, out, order, mode, cval, device)


def regrid_map(mins, delta, like_shape, like_mins, like_delta, rotation=None):
    """(matrix, offset) in float64 that take an index of the lattice (like_mins, like_delta) of `like_shape` to the index of the same
    world point on the lattice (mins, delta); rotation: the world point is first turned by this matrix about the target lattice's centre"""
    ndim = len(like_shape)
    mins = np.asarray(mins, dtype=np.float64).reshape(ndim)
    like_mins = np.asarray(like_mins, dtype=np.float64).reshape(ndim)
    delta = np.asarray(delta, dtype=np.float64) * np.ones(ndim)
    like_delta = np.asarray(like_delta, dtype=np.float64) * np.ones(ndim)
    assert np.all(delta != 0.0) and np.all(like_delta != 0.0), "a lattice step of 0"
    R = np.eye(ndim) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(ndim, ndim)
    centre = like_mins + like_delta * (np.asarray(like_shape, dtype=np.float64) - 1.0) / 2.0
    # world x = like_mins + like_delta i;  turned: centre + R (x - centre);  source index: (that - mins) / delta
    matrix = (R * like_delta[None, :]) / delta[:, None]
    offset = (centre + R @ (like_mins - centre) - mins) / delta
    return matrix, offset


def regrid(samples, mins, delta, like_shape, like_mins, like_delta, rotation=None, order=1, mode="constant", cval=0.0, device=None,
           return_map=False, return_outside=False):
    """the samples of the lattice (mins, delta) on the lattice (like_mins, like_delta) of `like_shape`: what makes a second volume a
    legal `field` of vertex_values and clip beside a marched volume of that shape.  rotation: an optional world rotation (ndim x ndim)
    about the target lattice's centre.  Matrix and offset are computed in float64 on the host (`regrid_map`).
    -> the result; with return_outside (result, n_outside); with return_map the matrix and the offset follow."""
    matrix, offset = regrid_map(mins, delta, like_shape, like_mins, like_delta, rotation)
    result, n_outside = resample(samples, matrix, offset, tuple(int(n) for n in like_shape), order, mode, cval, device, return_outside=True)
    out = (result, n_outside) if return_outside else (result,)
    if return_map:
        out = out + (matrix, offset)
    return out[0] if len(out) == 1 else out


def reslice(samples, origin, u, v, shape, order=1, mode="constant", cval=0.0, device=None, return_outside=False):
    """one oblique plane of a 3-D volume: the image out[i, j] = f(origin + i u + j v), origin, u and v in index coordinates of the
    samples, `shape` the image's (rows, columns)."""
    assert len(samples.shape) == 3, "reslice: a 3-D volume"
    matrix = np.zeros((3, 3))
    matrix[:, 1] = np.asarray(u, dtype=np.float64).reshape(3)
    matrix[:, 2] = np.asarray(v, dtype=np.float64).reshape(3)
    out = resample(samples, matrix, np.asarray(origin, dtype=np.float64).reshape(3), (1, int(shape[0]), int(shape[1])), order, mode, cval,
                   device, return_outside=True)
    image = out[0].reshape(int(shape[0]), int(shape[1]))
    return (image, out[1]) if return_outside else image


def lattice_after(mins, delta, matrix, offset):
    """world (mins, delta) of the result of `resample`, per axis of the RESULT, when the map is a scaled permutation (zoom, crop,
    regrid without rotation, flip, transpose): result axis k runs along the samples' axis a with M[a][k] != 0, from
    mins[a] + delta[a] offset[a] in steps of delta[a] M[a][k] (negative after a flip).  Asserts for any other matrix."""
    mins = np.asarray(mins, dtype=np.float64).reshape(-1)
    ndim = len(mins)
    delta = np.asarray(delta, dtype=np.float64) * np.ones(ndim)
    M = np.asarray(matrix, dtype=np.float64)
    if M.ndim < 2:
        M = np.diag(M * np.ones(ndim))
    off = np.asarray(offset, dtype=np.float64) * np.ones(ndim)
    assert M.shape == (ndim, ndim), "matrix: %d x %d" % (ndim, ndim)
    nz = M != 0.0
    assert np.all(nz.sum(axis=0) == 1) and np.all(nz.sum(axis=1) == 1), "lattice_after: the matrix is not a scaled permutation"
    new_mins, new_delta = np.zeros(ndim), np.zeros(ndim)
    for a in range(ndim):
        k = int(np.flatnonzero(nz[a])[0])
        new_mins[k] = mins[a] + delta[a] * off[a]
        new_delta[k] = delta[a] * M[a, k]
    return new_mins, new_delta


# ---- rank filters (cx_grid_rank3d, csrc/cx_rank.hip) ---------------------------------------------------------------------------------
# out[i] = the element at position `rank` of the sorted window {samples[src(i + d - origin)] : d in the footprint}, in the samples' own
# type: scipy.ndimage.rank_filter.  Nothing is computed, a sample is selected, so the result equals scipy's in value and a numpy
# restatement (tests/rank_ref.py) bit for bit.  Floats are ordered -inf < ... < -0.0 < +0.0 < ... < +inf < NaN; a selected NaN comes out
# as the canonical quiet NaN.  Modes "nearest", "reflect" and "constant" are scipy's 'nearest', 'reflect' and 'constant'.  `origin` is
# the offset of the footprint's box that sits on the output sample, 0 .. size - 1, None for the middle one (`default_origin`); scipy's
# `origin` argument is this one minus size // 2.  The result's lattice is the samples' own: the same (mins, delta),
# `lattice_of(mins, delta)` with no weights.

MAX_RANK_SIZE = 7      # per axis of cx_grid_rank3d


def ball(radius):
    "the boolean footprint {d : |d - c|^2 <= radius^2} in a box of side 2 int(radius) + 1 with centre c, for radius < 4"
    radius = float(radius)
    assert 0.0 <= radius < 4.0, "a radius of 0 to less than 4 (a box of at most %d per axis)" % MAX_RANK_SIZE
    r = int(radius)
    d = np.arange(-r, r + 1, dtype=np.float64) ** 2
    return d[:, None, None] + d[None, :, None] + d[None, None, :] <= radius * radius


def percentile_rank(percentile, n_window):
    "scipy.ndimage.percentile_filter's rank: a negative percentile has 100 added; 100 is the last element; else int(W p / 100.0)"
    p = percentile
    if p < 0.0:
        p += 100.0
    assert 0.0 <= p <= 100.0, "a percentile of -100 to 100"
    return int(n_window) - 1 if p == 100.0 else int(float(n_window) * p / 100.0)


def _rank_footprint(size, footprint, ndim):
    "(size, footprint) of an array of `ndim` axes -> (the box's three sides, the footprint as a 3-D bool array or None, W)"
    if footprint is None:
        box = [int(s) for s in _per_axis(size, ndim, 1, "size")]
        assert all(1 <= s <= MAX_RANK_SIZE for s in box), "a size of 1 to %d per axis" % MAX_RANK_SIZE
        return box, None, box[0] * box[1] * box[2]
    fp = np.asarray(footprint) != 0
    assert fp.ndim == ndim, "footprint: one axis per axis of the samples (%d)" % ndim
    fp = np.ascontiguousarray(fp.reshape((1,) * (3 - ndim) + fp.shape))
    assert all(1 <= s <= MAX_RANK_SIZE for s in fp.shape), "a footprint of 1 to %d per axis" % MAX_RANK_SIZE
    return [int(s) for s in fp.shape], fp, int(fp.sum())


def _rank_cval(cval, dtype):
    "cval as a value of the sample type: rounded to it for a float type, an integer in range for an integer type"
    name = str(dtype).replace("torch.", "")
    if name == "bfloat16":
        import torch
        return float(torch.tensor(float(cval), dtype=torch.float32).to(torch.bfloat16).float().item())
    dt = np.dtype(name)
    if dt.kind == "f":
        return float(np.asarray(cval, dtype=np.float64).astype(dt))
    info = np.iinfo(dt)
    assert float(cval) == int(cval) and info.min <= int(cval) <= info.max, "cval: an integer of the sample type (%s)" % dt.name
    return int(cval)


def rank_filter(samples, rank, size=3, footprint=None, origin=None, mode="nearest", cval=0, device=None):
    """scipy.ndimage.rank_filter(samples, rank, size or footprint, mode=mode, cval=cval, origin=origin - size // 2) in the samples' own
    type.  size: one side or one per axis, 1..7, ignored when a footprint (an array of the samples' dimensions, non-zero = in the
    window) is given; rank: 0 .. W - 1 among the W elements of the window, a negative one counts from the end.
    Samples: a numpy array (a numpy array comes back) or a contiguous GPU tensor (a tensor comes back) of 1 to 3 dimensions; bool
    samples count as uint8 0 and 1; types the kernels do not read are converted to float32 first.  The result lives on the samples' own
    lattice (`lattice_of(mins, delta)` with no weights)."""
    on_device, s, shape = _distance_samples(samples)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    box, fp, n_window = _rank_footprint(size, footprint, ndim)
    rank = int(rank)
    if rank < 0:
        rank += n_window
    og = [b // 2 for b in box] if origin is None else [int(o) for o in _per_axis(origin, ndim, 0, "origin")]
    fill = _rank_cval(cval, s.dtype)
    shape3 = (1,) * (3 - ndim) + shape
    if on_device:
        import torch
        context = _context(s.device.index if device is None else device)
        out = torch.empty(shape3, dtype=s.dtype, device=s.device)
        torch.cuda.current_stream(s.device).synchronize()      # the samples are there; the context has a stream of its own
        context.rank_grid(box, rank, fp, og, mode, fill, samples=(s.data_ptr(), s.dtype, shape3), out=out.data_ptr())
        return out.reshape(shape)
    context = _context(device)
    return context.rank_grid(box, rank, fp, og, mode, fill, samples=s.reshape(shape3), download=True)[1].reshape(shape)


def _n_window(samples, size, footprint):
    return _rank_footprint(size, footprint, len(samples.shape))[2]


def median(samples, size=3, footprint=None, origin=None, mode="nearest", cval=0, device=None):
    "scipy.ndimage.median_filter: rank W // 2 of `rank_filter`.  On a uint8 mask with an odd W: the majority filter"
    return rank_filter(samples, _n_window(samples, size, footprint) // 2, size, footprint, origin, mode, cval, device)


def minimum(samples, size=3, footprint=None, origin=None, mode="nearest", cval=0, device=None):
    "scipy.ndimage.minimum_filter (grey erosion by a flat footprint): rank 0 of `rank_filter`; separable, and computed so, for a whole box"
    return rank_filter(samples, 0, size, footprint, origin, mode, cval, device)


def maximum(samples, size=3, footprint=None, origin=None, mode="nearest", cval=0, device=None):
    "scipy.ndimage.maximum_filter (grey dilation by a flat footprint): rank W - 1 of `rank_filter`; separable, and computed so, for a whole box"
    return rank_filter(samples, -1, size, footprint, origin, mode, cval, device)


def percentile(samples, percentile, size=3, footprint=None, origin=None, mode="nearest", cval=0, device=None):
    "scipy.ndimage.percentile_filter: rank `percentile_rank(percentile, W)` of `rank_filter`"
    return rank_filter(samples, percentile_rank(percentile, _n_window(samples, size, footprint)), size, footprint, origin, mode, cval, device)


# ---- morphological reconstruction (cx_grid_reconstruct3d, csrc/cx_recon.hip) ----------------------------------------------------------
# Reconstruction by dilation of a marker g under a mask f: the largest R <= f above min(g, f) in which every sample is reached from it
# by a path of neighbours along which R does not increase; by erosion: the dual.  The result is made of minima and maxima of the
# samples only, in their own type, in the order of the rank filters (-inf < ... < -0.0 < +0.0 < ... < +inf < NaN), and equals a numpy
# restatement (tests/recon_ref.py) bit for bit.  connectivity 1, 2, 3: 6, 18 or 26 neighbours in three dimensions, as `label` counts
# them.  The result's lattice is the samples' own.

def _recon_faces(faces, ndim):
    "'all' or a mask of the bits 2 a (the low face of axis a of the samples) and 2 a + 1 (its high face) -> the bits of the padded shape"
    full = (1 << (2 * ndim)) - 1
    if isinstance(faces, str):
        assert faces == "all", "faces: 'all' or a mask of the bits 2 * axis (low face) and 2 * axis + 1 (high face)"
        faces = full
    faces = int(faces)
    assert 1 <= faces <= full, "faces: at least one face, bits 0 .. %d for samples of %d dimensions" % (2 * ndim - 1, ndim)
    return faces << (2 * (3 - ndim))


def _recon_h(h, dtype):
    "h as cx_grid_reconstruct3d takes it: finite and above 0, an integer for an integer type"
    h = float(h)
    assert np.isfinite(h) and h > 0.0, "h: finite and above 0"
    try:
        name = np.dtype(dtype).name
    except TypeError:      # a torch type, or its name
        name = str(dtype).replace("torch.", "")
    assert "float" in name or h == int(h), "h: an integer for samples of an integer type (%s)" % name
    return h


def _reconstruct(samples, marker, h, faces, method, connectivity, out_kind, device):
    "marker: the name of a marker kind, or the marker array -> the result beside the samples: a tensor for a tensor, else a numpy array"
    assert method in _ffi.RECON_METHODS, "method: 'dilation' or 'erosion'"
    assert connectivity in (1, 2, 3), "connectivity: 1, 2 or 3"
    on_device, s, shape = _distance_samples(samples)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    shape3 = (1,) * (3 - ndim) + shape
    m = None
    if not isinstance(marker, str):
        m_on_device, m, m_shape = _distance_samples(marker)
        assert m_on_device == on_device, "marker and mask: two numpy arrays or two GPU tensors"
        assert m_shape == shape, "marker: the shape of the mask"
        assert m.dtype == s.dtype, "marker: the type of the mask (%s)" % s.dtype
    elif marker == "shift":
        h = _recon_h(h, s.dtype)
    elif marker == "rim":
        faces = _recon_faces(faces, ndim)
    if on_device:
        import torch
        context = _context(s.device.index if device is None else device)
        out = torch.empty(shape3, dtype=s.dtype if out_kind == "values" else torch.uint8, device=s.device)
        torch.cuda.current_stream(s.device).synchronize()      # the samples are there; the context has a stream of its own
        context.reconstruct_grid(marker if m is None else (m.data_ptr(), m.dtype, shape3), h, faces, method, connectivity, out_kind,
                                 samples=(s.data_ptr(), s.dtype, shape3), out=out.data_ptr())
        return out.reshape(shape)
    context = _context(device)
    return context.reconstruct_grid(marker if m is None else m.reshape(shape3), h, faces, method, connectivity, out_kind,
                                    samples=s.reshape(shape3), download=True)[1].reshape(shape)


def reconstruct(marker, mask, method="dilation", connectivity=1, device=None):
    """skimage.morphology.reconstruction(marker, mask, method) in the mask's type.  The marker is clamped into the mask first: min(marker,
    mask) for "dilation", max(marker, mask) for "erosion".  marker and mask: two numpy arrays (a numpy array comes back) or two contiguous
    GPU tensors (a tensor comes back) of one shape of 1 to 3 dimensions and one type; bool counts as uint8, types the kernels do not
    read are converted to float32 first."""
    assert not isinstance(marker, str), "marker: an array of the mask's shape"
    return _reconstruct(mask, marker, 0.0, 0, method, connectivity, "values", device)


def h_maxima(samples, h, connectivity=1, device=None):
    """the samples with every bump shallower than h cut off: the reconstruction by dilation of samples - h under the samples.  Integer
    samples: h an integer, samples - h saturates; float samples: samples - h computed in float64 and rounded to the type once."""
    return _reconstruct(samples, "shift", h, 0, "dilation", connectivity, "values", device)


def h_minima(samples, h, connectivity=1, device=None):
    "the samples with every pit shallower than h filled: the reconstruction by erosion of samples + h above the samples"
    return _reconstruct(samples, "shift", h, 0, "erosion", connectivity, "values", device)


def h_domes(samples, h, connectivity=1, device=None):
    "uint8, 1 where `h_maxima` lowered a sample: the support of the domes"
    return _reconstruct(samples, "shift", h, 0, "dilation", connectivity, "changed", device)


def h_basins(samples, h, connectivity=1, device=None):
    "uint8, 1 where `h_minima` raised a sample: the support of the basins"
    return _reconstruct(samples, "shift", h, 0, "erosion", connectivity, "changed", device)


def regional_maxima(samples, connectivity=1, device=None):
    """uint8, 1 on the plateaus no neighbour of which is higher (skimage.morphology.local_maxima): the markers to put on a `distance`
    field before touching grains are split.  Every type, floats included: the marker is the sample's predecessor in the order.  A
    constant array is one maximum (all ones), the smallest value of an integer type included; only -inf everywhere gives zeros."""
    return _reconstruct(samples, "step", 0.0, 0, "dilation", connectivity, "changed", device)


def regional_minima(samples, connectivity=1, device=None):
    "uint8, 1 on the plateaus no neighbour of which is lower (skimage.morphology.local_minima)"
    return _reconstruct(samples, "step", 0.0, 0, "erosion", connectivity, "changed", device)


def fill_holes_grey(samples, connectivity=1, device=None):
    """every pit that is not connected to the array's rim filled to its brim: the reconstruction by erosion from the rim, in the samples'
    type.  On a mask of 0 and 1: scipy.ndimage.binary_fill_holes with generate_binary_structure(ndim, connectivity)."""
    return _reconstruct(samples, "rim", 0.0, "all", "erosion", connectivity, "values", device)


def clear_border_grey(samples, faces="all", connectivity=1, mask=False, device=None):
    """the reconstruction by dilation from the rim: what of the samples is connected to the faces `faces` ('all', or a mask of the bits
    2 * axis for the low and 2 * axis + 1 for the high face of an axis of the samples), in the samples' type; mask=True: uint8, 1 where
    a sample is NOT reached at its own height.  Grey clear-border is samples - result: that subtraction is arithmetic in the caller's
    type and is left to the caller."""
    return _reconstruct(samples, "rim", 0.0, faces, "dilation", connectivity, "changed" if mask else "values", device)


def propagate(seeds, mask, connectivity=1, device=None):
    "scipy.ndimage.binary_propagation(seeds, generate_binary_structure(ndim, connectivity), mask=mask) of bool or uint8 arrays: uint8 0 and 1"
    def binary(a):
        if grid_field._is_torch(a):
            import torch
            assert a.dtype in (torch.bool, torch.uint8), "seeds and mask: bool or uint8"
            return (a != 0).to(torch.uint8)
        a = np.asarray(a)
        assert a.dtype in (np.bool_, np.uint8), "seeds and mask: bool or uint8"
        return (a != 0).astype(np.uint8)
    return _reconstruct(binary(mask), binary(seeds), 0.0, 0, "dilation", connectivity, "values", device)


# ---- marker-based watershed (cx_grid_watershed3d, csrc/cx_watershed.hip) ------------------------------------------------------------
# The labels of the markers flooded over a relief, low values first ("rising") or high values first ("falling": a distance field is
# flooded from its maxima without being negated).  Every sample of the domain (inside the region, not NaN) takes the label of the
# marker whose flood arrives first by the cost (level, steps since that level was entered); exact ties go to the neighbour with the
# smaller linear index, a stated bias that makes the labels a pure function of the inputs (include/contourist_hip.h, "watershed").
# They equal a numpy restatement (tests/watershed_ref.py) byte for byte; skimage.segmentation.watershed and
# scipy.ndimage.watershed_ift break ties differently.  The labels' lattice is the samples' own.

def _beside(a, on_device, shape, kind, name):
    "markers (kind int32) or a region (kind uint8, non-zero = inside) that lives where the relief does, contiguous and of its shape"
    if on_device:
        import torch
        assert grid_field._is_torch(a) and a.is_cuda, "%s: a GPU tensor beside a relief on the GPU" % name
        assert tuple(int(n) for n in a.shape) == shape, "%s: the shape of the relief" % name
        t = (a != 0).to(torch.uint8) if kind == "uint8" else a.to(torch.int32)
        return t.contiguous()
    assert not grid_field._is_torch(a), "%s: a numpy array beside a numpy relief" % name
    a = np.asarray(a)
    assert a.shape == shape, "%s: the shape of the relief" % name
    if kind == "uint8":
        return np.ascontiguousarray(a != 0, dtype=np.uint8)
    assert a.dtype.kind in "iub", "%s: integer labels" % name
    return np.ascontiguousarray(a, dtype=np.int32)


def _on_device(context, arrays):
    "numpy arrays as byte tensors on the context's device (None stays None), there when this returns"
    import torch
    dev = torch.device("cuda", context.device)
    out = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).to(dev) for a in arrays]
    torch.cuda.current_stream(dev).synchronize()      # the context has a stream of its own
    return out


def _flood(context, on_device, src, shape, shape3, markers_ptr, region_ptr, connectivity, direction, like):
    "cx_grid_watershed3d on device inputs -> (labels beside the caller's relief: a tensor like `like`, or a numpy array; stats)"
    if on_device:
        import torch
        out = torch.empty(shape3, dtype=torch.int32, device=like.device)
        stats, _ = context.watershed_grid(markers_ptr, region_ptr, connectivity, direction, samples=src, out=out.data_ptr())
        return out.reshape(shape), stats
    stats, labels = context.watershed_grid(markers_ptr, region_ptr, connectivity, direction, samples=src, out_host=True)
    return labels.reshape(shape), stats


def watershed(relief, markers=None, region=None, connectivity=1, direction="rising", device=None, return_stats=False):
    """the int32 labels of `markers` flooded over the relief (cx_grid_watershed3d); with return_stats=True (labels, stats).
    markers: integers of the relief's shape, a value above 0 a label (one label may sit on many samples); None: the labelled regional
    minima of the relief ("rising") or maxima ("falling"), found with `regional_minima` / `regional_maxima` and `label`'s kernels at
    the same connectivity.  region: None, or an array of the relief's shape, non-zero = inside; samples outside it and NaN samples get
    0 and stop the flood.  connectivity 1, 2, 3: 6, 18 or 26 neighbours.  direction "rising": the flood starts at low values;
    "falling": at high ones.  Exact ties go to the neighbour with the smaller linear index.
    Relief, markers and region: numpy arrays (a numpy array comes back) or contiguous GPU tensors (a tensor comes back) of 1 to 3
    dimensions; a bool relief counts as uint8, types the kernels do not read are converted to float32 first.  Every step runs on the
    device of one context: no volume crosses to the host between them."""
    assert direction in _ffi.WATERSHED_DIRECTIONS, "direction: 'rising' or 'falling'"
    assert connectivity in (1, 2, 3), "connectivity: 1, 2 or 3"
    on_device, s, shape = _distance_samples(relief)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    shape3 = (1,) * (3 - ndim) + shape
    m = None if markers is None else _beside(markers, on_device, shape, "int32", "markers")
    g = None if region is None else _beside(region, on_device, shape, "uint8", "region")
    if on_device:
        import torch
        context = _context(s.device.index if device is None else device)
        torch.cuda.current_stream(s.device).synchronize()      # the inputs are there; the context has a stream of its own
        ds, dm, dg = s, m, g
    else:
        context = _context(device)
        ds, dm, dg = _on_device(context, [s, m, g])
    src = (ds.data_ptr(), s.dtype, shape3)
    if dm is None:
        _, extrema = context.reconstruct_grid("step", 0.0, 0, "erosion" if direction == "rising" else "dilation", connectivity, "changed", samples=src)
        _, markers_ptr = context.label_grid(0.5, "high", connectivity, samples=(extrema, "uint8", shape3))
    else:
        markers_ptr = dm.data_ptr()
    labels, stats = _flood(context, on_device, src, shape, shape3, markers_ptr, None if dg is None else dg.data_ptr(), connectivity, direction, s)
    return (labels, stats) if return_stats else labels


def split_touching(samples, value, h, side="high", connectivity=1, sampling=None, device=None):
    """int32 labels that separate the touching grains, cells or pores of the object {f >= value} (side "high") or {f < value} ("low"):
    the distance inside the object (`distance`), its `h_maxima` (bumps of the distance field shallower than h do not split an object;
    h in the distance's units, finite and above 0), their regional maxima labelled as markers, and a falling `watershed` of the distance
    field with the object as the region.  0 outside the object.  The whole chain runs on one context; nothing but the labels comes
    back.  Samples: a numpy array (a numpy array comes back) or a contiguous GPU tensor (a tensor comes back) of 1 to 3 dimensions."""
    assert side in _ffi.LABEL_SIDES, "side: 'high' or 'low'"
    assert connectivity in (1, 2, 3), "connectivity: 1, 2 or 3"
    h = _recon_h(h, np.float32)
    on_device, s, shape = _distance_samples(samples)
    ndim = len(shape)
    assert 1 <= ndim <= 3, "samples of 1 to 3 dimensions"
    shape3 = (1,) * (3 - ndim) + shape
    if sampling is not None:
        sampling = [float(x) for x in _per_axis(sampling, ndim, 1.0, "sampling")]
    if on_device:
        import torch
        context = _context(s.device.index if device is None else device)
        torch.cuda.current_stream(s.device).synchronize()      # the samples are there; the context has a stream of its own
        ds = s
    else:
        context = _context(device)
        ds, = _on_device(context, [s])
    src = (ds.data_ptr(), s.dtype, shape3)
    k, _ = context.label_grid(value, side, connectivity, samples=src)
    _, region_ptr = context.label_select(np.concatenate([[False], np.ones(k, dtype=bool)]))      # the object, uint8
    _, dist_ptr = context.distance_grid(value, "above" if side == "high" else "below", "float32", sampling, samples=src)
    field = (dist_ptr, "float32", shape3)
    _, flat_ptr = context.reconstruct_grid("shift", h, 0, "dilation", connectivity, "values", samples=field)
    _, maxima_ptr = context.reconstruct_grid("step", 0.0, 0, "dilation", connectivity, "changed", samples=(flat_ptr, "float32", shape3))
    _, markers_ptr = context.label_grid(0.5, "high", connectivity, samples=(maxima_ptr, "uint8", shape3))
    return _flood(context, on_device, field, shape, shape3, markers_ptr, region_ptr, connectivity, "falling", s)[0]


# ---- regions of a labelled volume (cx_grid_regions3d*, csrc/cx_regions.hip) ----------------------------------------------------------
# What reads the labels `split_touching`, `watershed` or `label` made, or any other int32 label array: one record per label (size, box,
# centroid sums, the extremes and sums of a second array), masks of chosen labels cropped to a box, relabelling through a table, the
# pairs of labels that share a face, and one surface per label at the cost of its box.  A label <= 0 is background.  Everything is
# exact and equals a numpy restatement (tests/regions_ref.py) except `vsum` of a float array, whose bound the header states.

def _region_labels(labels):
    "-> (on_device, the labels int32 and contiguous, their shape, the shape padded to three axes, the `labels` argument of the regions calls)"
    if grid_field._is_torch(labels):
        import torch
        assert labels.is_cuda, "labels: a numpy array or a GPU tensor"
        t = labels.to(torch.int32).contiguous()
        shape = tuple(int(n) for n in t.shape)
        assert 1 <= len(shape) <= 3, "labels of 1 to 3 dimensions"
        shape3 = (1,) * (3 - len(shape)) + shape
        torch.cuda.current_stream(t.device).synchronize()      # the labels are there; the context has a stream of its own
        return True, t, shape, shape3, (t.data_ptr(), shape3)
    a = np.asarray(labels)
    assert a.dtype.kind in "iub", "labels: integers"
    a = np.ascontiguousarray(a, dtype=np.int32)
    assert 1 <= a.ndim <= 3, "labels of 1 to 3 dimensions"
    shape3 = (1,) * (3 - a.ndim) + a.shape
    return False, a, a.shape, shape3, a.reshape(shape3)


def _region_context(on_device, t, device):
    return _context((t.device.index if on_device else None) if device is None else device)


def regions(labels, values=None, device=None):
    """one record (`_ffi.REGION_DTYPE`) per label 1 .. K of an integer label array, K its largest label; record c - 1 belongs to label c:
    voxels, first, sum, lo, hi, rim as `label(..., measures=True)` gives them (over the three axes of the padded shape) and, with
    `values` (an array of the labels' shape), n_nan, min_at / max_at (linear indices; ties: the smallest), vmin / vmax, isum, vsum.
    What scipy.ndimage.find_objects, sum, minimum_position and maximum_position give, in one pass.  A label nobody carries has
    voxels 0.  Labels and values: numpy arrays or contiguous GPU tensors of 1 to 3 dimensions; the records are a numpy array."""
    on_device, t, shape, shape3, arg = _region_labels(labels)
    context = _region_context(on_device, t, device)
    varg = None
    if values is not None:
        v_on_device, v, vshape = _distance_samples(values)
        assert vshape == shape, "values: the shape of the labels"
        if v_on_device:
            import torch
            torch.cuda.current_stream(v.device).synchronize()
            varg = (v.data_ptr(), v.dtype, shape3)
        else:
            varg = v.reshape(shape3)
    return context.regions_grid(arg, varg)


def _keep_flags(ids):
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    assert len(ids) == 0 or ids.min() >= 0, "ids: labels, 0 for the background"
    flags = np.zeros(int(ids.max()) + 1 if len(ids) else 1, dtype=np.uint8)
    flags[ids] = 1
    return flags


def region_mask(labels, ids, box=None, pad=0, device=None):
    """(uint8 mask, origin): 1 where the label is one of `ids` (0 names the background), cropped to the index box `box` = (lo, hi), both
    ends included (None: the whole array), grown by `pad` samples (0 .. 8) on every side of every axis; where that leaves the array the
    mask is 0.  origin = lo - pad: the index of the mask's first sample in the labels' array (negative where the pad leaves it).  A
    numpy array for numpy labels, a tensor for a tensor."""
    on_device, t, shape, shape3, arg = _region_labels(labels)
    context = _region_context(on_device, t, device)
    ndim, lead = len(shape), 3 - len(shape)
    lo3, hi3 = [0] * 3, [n - 1 for n in shape3]
    if box is not None:
        lo, hi = [list(np.asarray(b, dtype=np.int64).reshape(ndim)) for b in box]
        lo3[lead:], hi3[lead:] = [int(x) for x in lo], [int(x) for x in hi]
    pad = int(pad)
    ext = tuple(hi3[a] - lo3[a] + 1 + 2 * pad for a in range(3))
    if on_device:
        import torch
        out = torch.empty([max(0, e) for e in ext], dtype=torch.uint8, device=t.device)
        _, shape_out, origin, _ = context.regions_select(arg, _keep_flags(ids), (lo3, hi3), pad, out=out.data_ptr())
    else:
        _, shape_out, origin, out = context.regions_select(arg, _keep_flags(ids), (lo3, hi3), pad, download=True)
    assert tuple(out.shape) == shape_out
    for _ in range(lead):      # a padded leading axis has one real plane, at index pad
        out = out[pad]
    return out, tuple(origin[lead:])


def _mapped(context, on_device, t, shape, arg, table):
    "the labels through the table: a new tensor beside the labels, or a numpy array"
    if on_device:
        import torch
        out = torch.empty_like(t)
        context.regions_map(arg, table, out=out.data_ptr())
        return out
    return context.regions_map(arg, table, download=True).reshape(shape)


def relabel(labels, device=None):
    """(labels, forward_map): the labels renumbered 1 .. M in the order of their values, as skimage.segmentation.relabel_sequential
    does; forward_map[old] = new (int32, K + 1 entries, 0 for labels nobody carries and for the background)."""
    on_device, t, shape, shape3, arg = _region_labels(labels)
    context = _region_context(on_device, t, device)
    records = context.regions_grid(arg)
    forward = np.zeros(len(records) + 1, dtype=np.int32)
    present = records["voxels"] > 0
    forward[1:][present] = np.arange(1, int(present.sum()) + 1, dtype=np.int32)
    return _mapped(context, on_device, t, shape, arg, forward), forward


def keep_regions(labels, min_voxels=None, rim=None, keep=None, device=None):
    """the labels with the regions that fail a criterion set to 0; the others keep their ids.  min_voxels=n: at least n voxels;
    rim=True / False: only regions that touch / do not touch the array's rim (on an axis of the labels; padded leading axes do not
    count); keep: a bool array over the labels 1 .. K, or a callable that gets the records and returns one."""
    on_device, t, shape, shape3, arg = _region_labels(labels)
    context = _region_context(on_device, t, device)
    records = context.regions_grid(arg)
    k = len(records)
    ok = records["voxels"] > 0
    if min_voxels is not None:
        ok &= records["voxels"] >= int(min_voxels)
    if rim is not None:
        real = 0
        for axis in range(3 - len(shape), 3):
            real |= 3 << (2 * axis)
        touches = (records["rim"] & np.uint32(real)) != 0
        ok &= touches if rim else ~touches
    if keep is not None:
        flags = np.asarray(keep(records) if callable(keep) else keep).astype(bool).reshape(-1)
        assert len(flags) == k, "keep: one flag per label (%d)" % k
        ok &= flags
    table = np.zeros(k + 1, dtype=np.int32)
    table[1:][ok] = np.flatnonzero(ok) + 1
    return _mapped(context, on_device, t, shape, arg, table)


def contacts(labels, sampling=None, device=None):
    """the pairs of labels a < b that share a face somewhere (0, the background, included as a partner): records of
    `_ffi.REGION_CONTACT_DTYPE` sorted by (a, b), faces[x] = the sample pairs adjacent along axis x of the padded shape.  With
    `sampling` (the lattice steps, one or one per axis) the records get a column `area` = sum over x of faces[x] times the product of
    the two other steps (a missing leading axis has step 1)."""
    on_device, t, shape, shape3, arg = _region_labels(labels)
    context = _region_context(on_device, t, device)
    found = context.regions_contacts(arg)
    if sampling is None:
        return found
    steps = [1.0] * (3 - len(shape)) + [float(x) for x in _per_axis(sampling, len(shape), 1.0, "sampling")]
    out = np.zeros(len(found), dtype=np.dtype(_ffi.REGION_CONTACT_DTYPE.descr + [("area", "<f8")]))
    for name in ("a", "b", "faces"):
        out[name] = found[name]
    out["area"] = sum(found["faces"][:, x].astype(np.float64) * (steps[(x + 1) % 3] * steps[(x + 2) % 3]) for x in range(3))
    return out


def region_surfaces(labels, ids=None, mins=None, delta=None, pad=1, device=None):
    """a generator of (id, points float64 (V, 3), triangles int32 (T, 3)): the surface of every region of `ids` (None: every label some
    sample carries), each from its own box: the region's mask cropped to the record's box grown by `pad` (>= 1 closes the surface;
    the rim of the array counts as outside), bound, marched at 0.5 and post-processed.  Points are in the whole volume's coordinates:
    indices of the labels' array, or index * delta + mins when either is given.  The cost follows the boxes, not the number of
    labels times the volume.  Labels: a 3-D numpy array or GPU tensor.  The context's bound grid and extraction are replaced."""
    on_device, t, shape, shape3, arg = _region_labels(labels)
    assert len(shape) == 3, "3-D labels"
    context = _region_context(on_device, t, device)
    records = context.regions_grid(arg)
    if ids is None:
        ids = np.flatnonzero(records["voxels"] > 0) + 1
    scale = np.ones(3) if delta is None else np.asarray(delta, dtype=np.float64).reshape(3)
    shift = np.zeros(3) if mins is None else np.asarray(mins, dtype=np.float64).reshape(3)
    try:
        for c in [int(x) for x in np.asarray(ids).reshape(-1)]:
            if c < 1 or c > len(records) or records["voxels"][c - 1] == 0:
                yield c, np.zeros((0, 3), dtype=np.float64), np.zeros((0, 3), dtype=np.int32)
                continue
            flags = np.zeros(c + 1, dtype=np.uint8)
            flags[c] = 1
            _, _, origin, _ = context.regions_select(arg, flags, (records["lo"][c - 1], records["hi"][c - 1]), pad)
            context.bind_region_mask()
            context.set_origin(*origin)      # (the march's tie-breaks hash the volume's own lattice points)
            context.extract3d(0.5)
            post = context.postprocess3d()
            points, triangles = context.download_level1(post)
            if min(origin) >= 0:      # the post-pass works in the array's own coordinates unless the array starts before the volume
                points = points + np.asarray(origin, dtype=np.float64)
            if mins is not None or delta is not None:
                points = points * scale + shift
            yield c, points, triangles
    finally:
        context.set_origin(0, 0, 0)      # the module's context goes back to an array that starts at the volume's first sample
