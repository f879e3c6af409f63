"""numpy restatement of the regions calls (include/contourist_hip.h, section "regions"; csrc/cx_regions.hip): the records per label,
the cropped mask, the map and the face contacts, and the label patterns and value arrays the tests of both sides use.  Plain numpy,
written to be read: it is the contract's second statement."""
import math

import numpy as np

MAX_LABEL = 1 << 24      # CX_REGIONS_MAX_LABEL
GROUPS_MAX = 8           # CXR_GROUPS_MAX of cx_regions.hip: more labels than this in a tile of 64 columns take the per-lane path
TABLE_MIN_PAIRS = 512    # half of CXR_TABLE_MIN: more pairs than this overflow the first contact table of a fresh context

REGION_DTYPE = np.dtype([("voxels", "<i8"), ("first", "<i8"), ("sum", "<i8", (3,)), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                         ("rim", "<u4"), ("reserved", "<u4"), ("n_nan", "<i8"), ("min_at", "<i8"), ("max_at", "<i8"), ("vmin", "<f8"),
                         ("vmax", "<f8"), ("isum", "<i8"), ("vsum", "<f8")])
CONTACT_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("faces", "<i8", (3,))])
FLOAT_NAMES = ("float32", "float16", "bfloat16")
DTYPE_NAMES = ("float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16")


def background(labels):
    "the labels as the calls read them: a label <= 0 is 0"
    L = np.asarray(labels).astype(np.int64)
    assert L.ndim == 3
    return np.where(L > 0, L, 0)


def as_float64(values, name):
    "the samples as float64, exactly; bfloat16 arrives as its uint16 bit patterns"
    v = np.asarray(values)
    if name == "bfloat16":
        return (v.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return v.astype(np.float64)


def order_key(v):
    "float64 -> uint64 in the order -inf < ... < -0.0 < +0.0 < ... < +inf (no NaN comes here)"
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where((b >> np.uint64(63)) == 1, ~b, b | np.uint64(1 << 63))


def regions(labels, values=None, name=None, with_abs=False):
    """-> records (REGION_DTYPE), record c - 1 for label c, K = the largest label; with_abs: (records, sum |v| per label over the
    samples that are not NaN, as exact as math.fsum makes it): what the bound of a float vsum is made of.  vsum of a float array is
    math.fsum of the values: the correctly rounded sum."""
    L = background(labels)
    n0, n1, n2 = L.shape
    k = int(L.max())
    assert k <= MAX_LABEL
    out = np.zeros(k, dtype=REGION_DTYPE)
    out["first"] = -1
    out["hi"] = -1
    out["min_at"] = -1
    out["max_at"] = -1
    abs_sum = np.zeros(k, dtype=np.float64)
    flat = L.reshape(-1)
    at = np.flatnonzero(flat > 0)
    c = flat[at] - 1
    i, j, kk = np.unravel_index(at, L.shape)
    np.add.at(out["voxels"], c, 1)
    first = np.full(k, np.iinfo(np.int64).max)
    np.minimum.at(first, c, at)
    present = out["voxels"] > 0
    out["first"][present] = first[present]
    lo = np.full((k, 3), np.iinfo(np.int32).max, dtype=np.int64)
    hi = np.full((k, 3), -1, dtype=np.int64)
    rim = np.zeros(k, dtype=np.uint32)
    for axis, (x, n) in enumerate(((i, n0), (j, n1), (kk, n2))):
        np.add.at(out["sum"][:, axis], c, x)
        np.minimum.at(lo[:, axis], c, x)
        np.maximum.at(hi[:, axis], c, x)
        np.bitwise_or.at(rim, c[x == 0], np.uint32(1 << (2 * axis)))
        np.bitwise_or.at(rim, c[x == n - 1], np.uint32(2 << (2 * axis)))
    out["lo"][present] = lo[present]
    out["hi"][present] = hi[present]
    out["rim"] = rim
    if values is not None:
        name = name or str(np.asarray(values).dtype)
        v = as_float64(values, name).reshape(-1)[at]
        nan = np.isnan(v)
        np.add.at(out["n_nan"], c[nan], 1)
        cv, av, vv = c[~nan], at[~nan], v[~nan]
        key = order_key(vv)
        # the smallest value of every label, among equal values the smallest index; the largest value, again the smallest index
        for field_at, field_v, kkey in (("min_at", "vmin", key), ("max_at", "vmax", ~key)):
            order = np.lexsort((av, kkey, cv))
            heads = order[np.r_[True, cv[order][1:] != cv[order][:-1]]] if len(order) else order
            out[field_at][cv[heads]] = av[heads]
            out[field_v][cv[heads]] = vv[heads]
        order = np.argsort(cv, kind="stable")
        bounds = np.flatnonzero(np.r_[True, cv[order][1:] != cv[order][:-1], True]) if len(order) else np.zeros(1, dtype=np.int64)
        for s, e in zip(bounds[:-1], bounds[1:]):
            members = vv[order[s:e]]
            label = cv[order[s]]
            finite = members[np.isfinite(members)]
            abs_sum[label] = math.fsum(np.abs(finite))
            if name in FLOAT_NAMES:
                # (an infinity among the values makes the sum that infinity in any order, both of them NaN)
                with np.errstate(invalid="ignore"):
                    out["vsum"][label] = math.fsum(finite) + float(members[~np.isfinite(members)].sum())
            else:
                out["isum"][label] = int(members.astype(np.int64).sum())
                out["vsum"][label] = float(out["isum"][label])
    return (out, abs_sum) if with_abs else out


def vsum_bound(records, abs_sum):
    "the bound of a sum of doubles in any order, per label: (voxels - 1) * 2^-53 * sum |v|"
    return np.maximum(records["voxels"] - 1, 0) * 2.0 ** -53 * abs_sum


def select(labels, keep, box=None, pad=0):
    """-> (uint8 mask, origin, number of ones): keep[label] != 0 on the array extended by zeros, cropped to [lo - pad, hi + pad].
    One sample at a time: the statement.  select_fast is what the tests of large arrays use, and the host test holds the two equal."""
    L = background(labels)
    keep = np.asarray(keep).reshape(-1) != 0
    lo = np.zeros(3, dtype=np.int64) if box is None else np.asarray(box[0], dtype=np.int64)
    hi = np.asarray(L.shape, dtype=np.int64) - 1 if box is None else np.asarray(box[1], dtype=np.int64)
    assert np.all(lo >= 0) and np.all(hi < L.shape) and np.all(lo <= hi) and 0 <= pad <= 8
    kept = np.zeros(L.shape, dtype=np.uint8)
    inside = L < len(keep)
    kept[inside] = keep[L[inside]]
    out = np.zeros(tuple(hi - lo + 1 + 2 * pad), dtype=np.uint8)
    for idx in np.ndindex(*out.shape):      # (the pad shows the array where it has samples there, zeros where it has none)
        src = np.asarray(idx) + lo - pad
        if np.all(src >= 0) and np.all(src < L.shape):
            out[idx] = kept[tuple(src)]
    return out, tuple(int(x) for x in lo - pad), int(out.sum())


def select_fast(labels, keep, box=None, pad=0):
    "the same without the loop over samples: the array padded by zeros, then cropped"
    L = background(labels)
    keep = np.asarray(keep).reshape(-1) != 0
    lo = np.zeros(3, dtype=np.int64) if box is None else np.asarray(box[0], dtype=np.int64)
    hi = np.asarray(L.shape, dtype=np.int64) - 1 if box is None else np.asarray(box[1], dtype=np.int64)
    assert np.all(lo >= 0) and np.all(hi < L.shape) and np.all(lo <= hi) and 0 <= pad <= 8
    kept = np.zeros(L.shape, dtype=np.uint8)
    inside = L < len(keep)
    kept[inside] = keep[L[inside]]
    wide = np.pad(kept, pad)
    out = np.ascontiguousarray(wide[lo[0]:hi[0] + 1 + 2 * pad, lo[1]:hi[1] + 1 + 2 * pad, lo[2]:hi[2] + 1 + 2 * pad])
    return out, tuple(int(x) for x in lo - pad), int(out.sum())


def relabel(labels, table):
    "out = table[label] for a label below len(table) (negative labels count as 0), else 0"
    L = background(labels)
    table = np.asarray(table, dtype=np.int32).reshape(-1)
    out = np.zeros(L.shape, dtype=np.int32)
    inside = L < len(table)
    out[inside] = table[L[inside]]
    return out


def contacts(labels):
    "-> records (CONTACT_DTYPE) sorted by (a, b): the pairs a < b of labels, 0 included, that are face neighbours; faces per axis"
    L = background(labels)
    found = {}
    for axis in range(3):
        near = np.take(L, np.arange(0, L.shape[axis] - 1), axis=axis).reshape(-1)
        far = np.take(L, np.arange(1, L.shape[axis]), axis=axis).reshape(-1)
        differ = near != far
        a, b = np.minimum(near, far)[differ], np.maximum(near, far)[differ]
        pairs, counts = np.unique((a << 32) | b, return_counts=True)
        for p, n in zip(pairs, counts):
            found.setdefault(int(p), [0, 0, 0])[axis] = int(n)
    out = np.zeros(len(found), dtype=CONTACT_DTYPE)
    for r, p in enumerate(sorted(found)):
        out[r] = (p >> 32, p & 0xFFFFFFFF, found[p])
    return out


# ---- the inputs of the tests ----------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (2, 2, 2), (1, 8, 9), (5, 4, 3), (3, 5, 63), (3, 5, 64), (2, 6, 65), (2, 3, 131), (37, 33, 259)]
STRADDLE = SHAPES[-1]
PATTERNS = ("voronoi5", "voronoi200", "voronoi5_zero", "voronoi200_zero", "noise", "one", "zeros", "gaps", "negative")


def voronoi(shape, seeds, rng):
    "nearest-seed labels 1 .. seeds (ties to the smaller label): no zeros between the regions"
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    centres = rng.uniform(size=(seeds, 3)) * np.asarray(shape)
    best = np.full(len(grid), np.inf)
    out = np.zeros(len(grid), dtype=np.int32)
    for s in range(seeds):
        d = ((grid - centres[s]) ** 2).sum(axis=1)
        closer = d < best
        best[closer] = d[closer]
        out[closer] = s + 1
    return out.reshape(shape)


def pattern(shape, kind, seed=0):
    "an int32 label array of `shape`"
    rng = np.random.RandomState(1000 + seed + sum(shape))
    if kind.startswith("voronoi"):
        L = voronoi(shape, 200 if "200" in kind else 5, rng)
        if kind.endswith("_zero"):
            L[voronoi(shape, 3, rng) == 2] = 0
        return L
    if kind == "noise":
        return rng.randint(0, 301, size=shape).astype(np.int32)
    if kind == "one":
        return np.full(shape, 3, dtype=np.int32)
    if kind == "zeros":
        return np.zeros(shape, dtype=np.int32)
    if kind == "gaps":
        return (voronoi(shape, 9, rng) * 7).astype(np.int32)
    if kind == "negative":
        L = voronoi(shape, 5, rng)
        L[rng.uniform(size=shape) < 0.2] = -4
        L[rng.uniform(size=shape) < 0.05] = np.iinfo(np.int32).min
        return L
    raise ValueError(kind)


def typed_values(shape, name, seed=0):
    """values of the sample type `name` over `shape` -> (the array as numpy holds it (bfloat16: uint16 bits), name).  Few distinct
    values, so that minima and maxima tie; floats carry NaN, both infinities and both zeros."""
    rng = np.random.RandomState(2000 + seed + sum(shape))
    n = int(np.prod(shape))
    if name in FLOAT_NAMES:
        pool = np.array([-np.inf, -2.5, -1.0, -0.0, 0.0, 0.5, 3.0, np.inf, np.nan], dtype=np.float32)
        v = pool[rng.randint(0, len(pool), size=n)]
        if name == "float16":
            return v.astype(np.float16).reshape(shape), name
        if name == "bfloat16":
            return (v.view(np.uint32) >> 16).astype(np.uint16).reshape(shape), name
        return v.reshape(shape), name
    info = np.iinfo(name)
    pool = np.array([info.min, info.min + 1, 0, 1, 7, info.max - 1, info.max], dtype=np.int64)
    return pool[rng.randint(0, len(pool), size=n)].astype(name).reshape(shape), name


def zeros_only(shape, name):
    "-0.0 and +0.0 alternating, -0.0 LAST in every pair of columns: vmin is -0.0 at an odd index, vmax +0.0 at an even one"
    v = np.zeros(shape, dtype=np.float32)
    v.reshape(-1)[1::2] = -0.0
    if name == "float16":
        return v.astype(np.float16)
    if name == "bfloat16":
        return (v.view(np.uint32) >> 16).astype(np.uint16)
    return v
