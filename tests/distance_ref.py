"""numpy restatement of cx_grid_distance3d (include/contourist_hip.h, "distance fields"): a sample f is LOW iff float64(f) < value (a NaN
is never low); the squared distance is a minimum per axis, last axis first, over every candidate of the axis, of
fl(g + fl(w (a - b)^2)) in float64 with w = s * s rounded once and (a - b)^2 the exact integer.  Brute force: one pass over the whole
array per candidate position, nothing skipped.  The morphology helpers of contourist_amd.volume are restated from it."""
import numpy as np

SIDES = ("below", "above", "signed")


def low_mask(samples, value):
    "samples: any type numpy converts to float64 exactly (bfloat16 goes in as its float32 values)"
    with np.errstate(invalid="ignore"):
        return np.asarray(samples).astype(np.float64) < np.float64(value)


def weights(sampling):
    s = np.ones(3, dtype=np.float64) if sampling is None else np.asarray(sampling, dtype=np.float64).reshape(3)
    return s * s


def axis_min(g, axis, w):
    "out[.., a, ..] = min over b of fl(g[.., b, ..] + fl(w (a - b)^2))"
    n = g.shape[axis]
    out = np.full(g.shape, np.inf, dtype=np.float64)
    pos = np.arange(n, dtype=np.int64)
    bshape = [1, 1, 1]
    bshape[axis] = n
    for b in range(n):
        cost = np.float64(w) * ((pos - b) ** 2).astype(np.float64)
        cand = np.take(g, [b], axis=axis) + cost.reshape(bshape)
        out = np.minimum(out, cand)
    return out


def transform(sites, sampling=None):
    "squared distance to the nearest True of the 3-D bool array `sites` (+inf without one), float64"
    sites = np.asarray(sites, dtype=bool)
    assert sites.ndim == 3
    w = weights(sampling)
    g = np.where(sites, np.float64(0.0), np.float64(np.inf))
    for axis in (2, 1, 0):
        g = axis_min(g, axis, w[axis])
    return g


def both(samples, value, sampling=None):
    "(gA, gB): the squared distances of side 'above' (sites: the low samples) and of side 'below' (sites: the others)"
    low = low_mask(samples, value)
    return transform(low, sampling), transform(~low, sampling)


def squared(samples, value, side="below", sampling=None, parts=None):
    gA, gB = both(samples, value, sampling) if parts is None else parts
    return gB if side == "below" else gA if side == "above" else gA - gB


def distance(samples, value, side="below", sampling=None, parts=None):
    gA, gB = both(samples, value, sampling) if parts is None else parts
    if side == "signed":
        return (np.sqrt(gA) - np.sqrt(gB)).astype(np.float32)
    return np.sqrt(gB if side == "below" else gA).astype(np.float32)


def mask(samples, value, side, radius2, sampling=None, parts=None):
    assert side in ("below", "above")
    return (squared(samples, value, side, sampling, parts) <= np.float64(radius2)).astype(np.uint8)


def n_sites(samples, value, side):
    low = int(low_mask(samples, value).sum())
    high = int(np.asarray(samples).size) - low
    return high if side == "below" else low if side == "above" else min(low, high)


def _r2(radius):
    return np.float64(float(radius) * float(radius))


def dilate(samples, value, radius, sampling=None):
    return mask(samples, value, "below", _r2(radius), sampling)


def erode(samples, value, radius, sampling=None):
    return np.uint8(1) - mask(samples, value, "above", _r2(radius), sampling)


def opened(samples, value, radius, sampling=None):
    return dilate(erode(samples, value, radius, sampling), 0.5, radius, sampling)


def closed(samples, value, radius, sampling=None):
    return erode(dilate(samples, value, radius, sampling), 0.5, radius, sampling)


def pad3(a):
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)
