"""cx_grid_label3d (include/contourist_hip.h, section "labels") restated in numpy alone: the labels with their numbering, the records,
the select and the functions of contourist_amd.volume built on them.

The labels: every labelled sample starts with its own linear index; a sweep gives each the minimum over itself and its labelled
neighbours (the offsets of the structure, never wrapping), then follows the indices it holds a few times (an index a sample holds
is a sample of its own component with a smaller index, so what THAT sample holds is one too).  At the fixed point every sample holds
the smallest linear index of its component; numbering those in ascending order is the contract's numbering."""
import itertools

import numpy as np

SIDES = ("high", "low")
RECORD_DTYPE = np.dtype([("voxels", "<i8"), ("first", "<i8"), ("sum", "<i8", (3,)), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                         ("rim", "<u4"), ("reserved", "<u4")])


def as3d(A):
    A = np.asarray(A)
    assert 1 <= A.ndim <= 3
    return A.reshape((1,) * (3 - A.ndim) + A.shape)


def labelled(A, value, side="high"):
    "the samples that get a label: a sample is LOW iff float64(f) < value (a NaN is never low)"
    A = np.asarray(A)
    if A.dtype == np.bool_:
        A = A.view(np.uint8)
    with np.errstate(invalid="ignore"):
        low = A.astype(np.float64) < np.float64(value)
    return low if side == "low" else ~low


def offsets(connectivity):
    "the neighbours: offsets in {-1, 0, 1}^3 that differ from 0 on 1 .. connectivity axes (6, 18, 26)"
    assert connectivity in (1, 2, 3)
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 1 <= sum(x != 0 for x in d) <= connectivity]


def _views(shape, d):
    "slices (dst, src) with src = dst + d inside the array"
    dst, src = [], []
    for n, x in zip(shape, d):
        if x == 0:
            dst.append(slice(0, n)); src.append(slice(0, n))
        elif x > 0:
            dst.append(slice(0, n - 1)); src.append(slice(1, n))
        else:
            dst.append(slice(1, n)); src.append(slice(0, n - 1))
    return tuple(dst), tuple(src)


def label_mask(M, connectivity=1):
    "(labels int32, K) of a bool array of 1 to 3 dimensions; `sweeps` of the last call in label_mask.sweeps"
    shape = np.asarray(M).shape
    M = as3d(np.asarray(M, dtype=bool))
    n = M.size
    idx = np.arange(n, dtype=np.int64).reshape(M.shape)
    L = np.where(M, idx, n)
    pairs = [_views(M.shape, d) for d in offsets(connectivity)]
    flatM = M.reshape(-1)
    where = np.flatnonzero(flatM)
    sweeps = 0
    while True:
        sweeps += 1
        new = L.copy()
        for dst, src in pairs:
            np.minimum(new[dst], L[src], out=new[dst])
        new[~M] = n
        flat = new.reshape(-1)
        for _ in range(3):
            flat[where] = flat[flat[where]]
        if np.array_equal(new, L):
            break
        L = new
    label_mask.sweeps = sweeps
    flat = L.reshape(-1)
    roots = np.zeros(n, dtype=np.int64)
    roots[where] = flat[where] == where
    rank = np.cumsum(roots)      # a root's rank, counted from 1
    out = np.zeros(n, dtype=np.int32)
    out[where] = rank[flat[where]]
    return out.reshape(shape), int(rank[-1]) if n else 0


label_mask.sweeps = 0


def label(A, value, side="high", connectivity=1):
    return label_mask(labelled(A, value, side), connectivity)


def records(labels, k):
    "one record per component of labels 1..k, every field an exact integer"
    L = as3d(labels)
    out = np.zeros(k, dtype=RECORD_DTYPE)
    if k == 0:
        return out
    flat = L.reshape(-1)
    where = np.flatnonzero(flat)
    c = flat[where].astype(np.int64) - 1
    out["voxels"] = np.bincount(c, minlength=k)
    first = np.full(k, flat.size, dtype=np.int64)
    np.minimum.at(first, c, where)
    out["first"] = first
    coords = np.unravel_index(where, L.shape)
    rim = np.zeros(k, dtype=np.uint32)
    for a in range(3):
        x = coords[a].astype(np.int64)
        s = np.zeros(k, dtype=np.int64)
        np.add.at(s, c, x)
        out["sum"][:, a] = s
        lo = np.full(k, np.iinfo(np.int32).max, dtype=np.int64)
        hi = np.full(k, np.iinfo(np.int32).min, dtype=np.int64)
        np.minimum.at(lo, c, x)
        np.maximum.at(hi, c, x)
        out["lo"][:, a] = lo
        out["hi"][:, a] = hi
        rim |= np.where(lo == 0, np.uint32(1 << (2 * a)), np.uint32(0)) | np.where(hi == L.shape[a] - 1, np.uint32(2 << (2 * a)), np.uint32(0))
    out["rim"] = rim
    return out


def select(labels, keep):
    "(uint8 mask, number of ones): 1 where keep[label] is set; keep has K + 1 entries, keep[0] for the samples without a label"
    flags = (np.asarray(keep) != 0).astype(np.uint8).reshape(-1)
    mask = flags[np.asarray(labels)]
    return mask, int(mask.sum())


def _real_rim(ndim):
    "the rim bits of the axes the samples have (padded leading axes do not count)"
    bits = 0
    for axis in range(3 - ndim, 3):
        bits |= 3 << (2 * axis)
    return np.uint32(bits)


def keep_components(A, value, side="high", connectivity=1, largest=None, min_voxels=None, rim=None, keep=None):
    A = np.asarray(A)
    labels, k = label(A, value, side, connectivity)
    rec = records(labels, k)
    ok = np.ones(k, dtype=bool)
    if min_voxels is not None:
        ok &= rec["voxels"] >= min_voxels
    if rim is not None:
        touches = (rec["rim"] & _real_rim(A.ndim)) != 0
        ok &= touches if rim else ~touches
    if keep is not None:
        ok &= np.asarray(keep(rec) if callable(keep) else keep).astype(bool).reshape(-1)
    if largest is not None:
        cand = [int(c) for c in np.flatnonzero(ok)]
        cand.sort(key=lambda c: (-int(rec["voxels"][c]), c))
        ok = np.zeros(k, dtype=bool)
        ok[cand[:largest]] = True
    return select(labels, np.concatenate([[False], ok]))[0]


def remove_small(A, value, min_voxels, connectivity=1):
    return keep_components(A, value, "high", connectivity, min_voxels=min_voxels)


def clear_border(A, value, connectivity=1):
    return keep_components(A, value, "high", connectivity, rim=False)


def fill_holes(A, value, connectivity=1):
    A = np.asarray(A)
    labels, k = label(A, value, "low", connectivity)
    rec = records(labels, k)
    enclosed = (rec["rim"] & _real_rim(A.ndim)) == 0
    return select(labels, np.concatenate([[True], enclosed]))[0]
