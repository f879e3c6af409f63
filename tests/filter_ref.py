"""numpy restatement of cx_grid_filter3d (include/contourist_hip.h, "preparing the volume"): per axis a loop over the taps, summed in
float64 with k ascending from +0.0, rounded to float32 once per pass; the passes run axis 2, axis 1, axis 0 with float32 between them.
The product of two float32 numbers is exact in float64, so numpy's multiply-then-add gives the double a fused multiply-add gives.
It carries its own weight builders: the tests compare contourist_amd.volume's against them bit for bit."""
import numpy as np

MODES = ("nearest", "reflect", "constant")
PYRAMID = np.asarray([1.0, 4.0, 6.0, 4.0, 1.0], dtype=np.float64) / 16.0


def src(j, n, mode):
    "(index read, outside) for the positions j of an axis of length n"
    j = np.asarray(j, dtype=np.int64)
    outside = (j < 0) | (j >= n)
    if mode == "nearest":
        return np.clip(j, 0, n - 1), np.zeros_like(outside)
    if mode == "reflect":
        p = np.mod(j, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p), np.zeros_like(outside)
    assert mode == "constant"
    return np.where(outside, 0, j), outside


def filter_axis(x, axis, weights, origin, stride, mode, cval):
    x = np.asarray(x)
    assert x.dtype == np.float32
    n = x.shape[axis]
    m = -(-n // stride)
    first = np.arange(m, dtype=np.int64) * stride
    if weights is None or len(weights) == 0:
        return np.ascontiguousarray(np.take(x, first, axis=axis))
    w = np.asarray(weights, dtype=np.float32)
    shape = list(x.shape)
    shape[axis] = m
    acc = np.zeros(shape, dtype=np.float64)
    bshape = [1, 1, 1]
    bshape[axis] = m
    with np.errstate(all="ignore"):
        for k in range(len(w)):
            idx, outside = src(first + k - origin, n, mode)
            v = np.take(x, idx, axis=axis).astype(np.float64)
            if mode == "constant":
                v = np.where(outside.reshape(bshape), np.float64(np.float32(cval)), v)
            acc = acc + np.float64(w[k]) * v
        return acc.astype(np.float32)


def filter3d(samples, axes, mode="nearest", cval=0.0):
    "samples: 3-D, any type numpy converts to float32 exactly; axes: three of (weights or None, origin, stride) -> float32"
    x = np.ascontiguousarray(np.asarray(samples).astype(np.float32))
    assert x.ndim == 3
    for axis in (2, 1, 0):
        w, origin, stride = axes[axis]
        x = filter_axis(x, axis, w, origin, stride, mode, cval)
    return x


def centre(n_weights):
    return n_weights // 2


def gaussian_weights(sigma, truncate=4.0):
    "scipy.ndimage._filters._gaussian_kernel1d of order 0, rounded to float32; None for sigma 0"
    if sigma == 0:
        return None
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)
    return (phi / phi.sum()).astype(np.float32)


def block_weights(factor):
    return None if factor == 1 else np.full(factor, 1.0 / factor, dtype=np.float64).astype(np.float32)


def three(v):
    return [v, v, v] if np.ndim(v) == 0 else list(v)


def gaussian(samples, sigma, truncate=4.0, stride=1, mode="nearest", cval=0.0):
    rows = [gaussian_weights(s, truncate) for s in three(sigma)]
    return filter3d(samples, [(w, 0 if w is None else centre(len(w)), s) for w, s in zip(rows, three(stride))], mode, cval)


def block_mean(samples, factor, mode="nearest", cval=0.0):
    return filter3d(samples, [(block_weights(f), 0, f) for f in three(factor)], mode, cval)


def pyramid(samples, levels, mode="nearest", cval=0.0):
    out = [np.asarray(samples)]
    w = PYRAMID.astype(np.float32)
    for _ in range(levels - 1):
        out.append(filter3d(out[-1], [(w, 2, 2) if n >= 2 else (None, 0, 1) for n in out[-1].shape], mode, cval))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    "bit for bit, a NaN for a NaN"
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(bits(got)[~gn], bits(want)[~wn]))
