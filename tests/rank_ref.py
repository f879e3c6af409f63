"""numpy restatement of cx_grid_rank3d (include/contourist_hip.h, "rank filters"): every sample becomes an unsigned key whose order is
the header's order and which has an inverse, the window of every output is gathered as one array over the footprint's offsets with the
boundary rule applied, np.sort puts it in ascending order, and the key at `rank` is turned back into a sample.  Written from the
header, not from the kernels; not imported by product code."""
import numpy as np

MODES = ("nearest", "reflect", "constant")
FLOATS = {"float32": (np.uint32, 32, 0x7F800000, 0x7FC00000), "float16": (np.uint16, 16, 0x7C00, 0x7E00), "bfloat16": (np.uint16, 16, 0x7F80, 0x7FC0)}
TYPES = ("float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16")


def type_name(a, dtype=None):
    "the sample type's name; dtype='bfloat16': `a` holds the uint16 bit patterns of bfloat16 samples"
    if dtype is not None and str(dtype).endswith("bfloat16"):
        assert np.asarray(a).dtype == np.uint16
        return "bfloat16"
    name = np.asarray(a).dtype.name
    assert name in TYPES and name != "bfloat16", name
    return name


def key(a, dtype=None):
    """the keys of the samples, unsigned integers of the samples' width.  Integers: the value with the sign bit flipped.  Floats: every
    NaN all ones; negative values all bits inverted, the others the sign bit set: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN"""
    a = np.ascontiguousarray(a)
    name = type_name(a, dtype)
    if name in FLOATS:
        U, bits, inf, _ = FLOATS[name]
        u = a.view(U)
        sign, ones = U(1 << (bits - 1)), U((1 << bits) - 1)
        k = np.where((u & sign) != 0, ~u, u | sign)
        k[(u & U(sign - 1)) > U(inf)] = ones
        return k
    U = np.dtype("u%d" % a.dtype.itemsize).type
    u = a.view(U)
    return u ^ U(1 << (8 * a.dtype.itemsize - 1)) if a.dtype.kind == "i" else u.copy()


def unkey(k, name):
    "the samples the keys stand for, in the numpy type of `name` (bfloat16: uint16 bit patterns); the NaN key: the canonical quiet NaN"
    k = np.ascontiguousarray(k)
    if name in FLOATS:
        U, bits, _, qnan = FLOATS[name]
        assert k.dtype == U
        sign, ones = U(1 << (bits - 1)), U((1 << bits) - 1)
        u = np.where((k & sign) != 0, k ^ sign, ~k)
        u[k == ones] = U(qnan)
        return u if name == "bfloat16" else u.view(np.dtype(name))
    dt = np.dtype(name)
    return (k ^ k.dtype.type(1 << (8 * dt.itemsize - 1))).view(dt) if dt.kind == "i" else k.view(dt)


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


def fill_key(cval, name):
    "the key of cval, which must be finite and a value of the sample type"
    assert np.isfinite(cval)
    if name == "bfloat16":
        b = np.asarray([cval], dtype=np.float32).view(np.uint32)
        assert (b[0] & 0xFFFF) == 0 and float(np.float32(cval)) == float(cval)
        return key((b >> 16).astype(np.uint16), "bfloat16")[0]
    with np.errstate(all="ignore"):
        v = np.asarray([cval]).astype(np.dtype(name))
    assert float(v[0]) == float(cval), (cval, name)
    return key(v)[0]


def box_of(size, footprint):
    "(the three sides, the footprint as a bool array of that shape)"
    if footprint is None:
        box = tuple(int(s) for s in (size if np.ndim(size) else [size] * 3))
        return box, np.ones(box, dtype=bool)
    fp = np.asarray(footprint) != 0
    assert fp.ndim == 3
    return fp.shape, fp


def sorted_windows(samples, size=3, footprint=None, origin=None, mode="nearest", cval=0, dtype=None):
    """the sorted keys of every window: an array (W, n0, n1, n2).  samples: 3-D; origin: None = size // 2, else the offset of the box
    that sits on the output sample, per axis"""
    A = np.ascontiguousarray(samples)
    assert A.ndim == 3
    name = type_name(A, dtype)
    box, fp = box_of(size, footprint)
    og = [s // 2 for s in box] if origin is None else [int(o) for o in origin]
    assert all(1 <= s <= 7 and 0 <= o < s for s, o in zip(box, og)) and fp.any()
    K = key(A, dtype)
    fill = fill_key(cval, name)
    windows = []
    for d in np.argwhere(fp):      # C order
        idx, off = [], []
        for a in range(3):
            j, outside = src(np.arange(A.shape[a]) + int(d[a]) - og[a], A.shape[a], mode)
            idx.append(j)
            off.append(outside)
        w = K[np.ix_(*idx)]
        outside = off[0][:, None, None] | off[1][None, :, None] | off[2][None, None, :]
        windows.append(np.where(outside, fill, w))
    return np.sort(np.stack(windows), axis=0)


def pick(ordered, rank, name):
    "the element at `rank` of every sorted window, as samples"
    assert 0 <= rank < len(ordered)
    return unkey(ordered[rank], name)


def rank_filter(samples, rank, size=3, footprint=None, origin=None, mode="nearest", cval=0, dtype=None):
    "cx_grid_rank3d of 3-D samples; a negative rank counts from the end, as scipy's does"
    ordered = sorted_windows(samples, size, footprint, origin, mode, cval, dtype)
    return pick(ordered, rank + len(ordered) if rank < 0 else rank, type_name(samples, dtype))


def pad3(a):
    "an array of 1 to 3 axes with leading axes of length 1: the padding rule of contourist_amd.volume"
    a = np.asarray(a)
    return a.reshape((1,) * (3 - a.ndim) + a.shape)


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()
