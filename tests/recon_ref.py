"""numpy restatement of cx_grid_reconstruct3d (include/contourist_hip.h, "reconstruction"): every sample becomes the unsigned key of the
rank filters (rank_ref.key), reconstruction by erosion works on the complemented keys, the marker is built from the mask by its kind and
clamped under the mask, and "dilate by the structure of the connectivity, take the minimum with the mask" is repeated until nothing
moves.  Written from the header, not from the kernels; not imported by product code."""
import numpy as np

import rank_ref as R

METHODS = ("dilation", "erosion")
KINDS = ("array", "shift", "step", "rim")
ALL_FACES = 63


def ones_of(K):
    return K.dtype.type(np.iinfo(K.dtype).max)


def offsets(connectivity):
    "the neighbours of a sample: the offsets that differ from it on 1 .. connectivity axes"
    assert connectivity in (1, 2, 3)
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < abs(a) + abs(b) + abs(c) <= connectivity]


def dilate(V, connectivity):
    "the maximum over every sample and its neighbours; outside the array lies the bottom of the order"
    n0, n1, n2 = V.shape
    P = np.zeros((n0 + 2, n1 + 2, n2 + 2), dtype=V.dtype)
    P[1:-1, 1:-1, 1:-1] = V
    out = V.copy()
    for a, b, c in offsets(connectivity):
        np.maximum(out, P[1 + a:1 + a + n0, 1 + b:1 + b + n1, 1 + c:1 + c + n2], out=out)
    return out


def iterate(G, F, connectivity):
    "the reconstruction by dilation of the keys G <= F under F"
    V = G.copy()
    while True:
        nxt = np.minimum(F, dilate(V, connectivity))
        if np.array_equal(nxt, V):
            return V
        V = nxt


def raster(G, F, connectivity):
    "the same by sequential sweeps in raster and anti-raster order until a pair of sweeps moves nothing (small arrays only)"
    V = G.copy()
    n = V.shape
    nb = offsets(connectivity)
    order = [(i, j, k) for i in range(n[0]) for j in range(n[1]) for k in range(n[2])]
    while True:
        moved = False
        for sweep in (order, order[::-1]):
            for i, j, k in sweep:
                best = V[i, j, k]
                for a, b, c in nb:
                    p, q, r = i + a, j + b, k + c
                    if 0 <= p < n[0] and 0 <= q < n[1] and 0 <= r < n[2] and V[p, q, r] > best:
                        best = V[p, q, r]
                best = min(best, F[i, j, k])
                if best != V[i, j, k]:
                    V[i, j, k] = best
                    moved = True
        if not moved:
            return V


def ends(name):
    "(the key of the smallest, of the largest sample that is no NaN, whether the type has NaNs)"
    if name in R.FLOATS:
        U, bits, inf, _ = R.FLOATS[name]
        b = np.array([inf | (1 << (bits - 1)), inf], dtype=U)
        k = R.key(b if name == "bfloat16" else b.view(np.dtype(name)), "bfloat16" if name == "bfloat16" else None)
        return k[0], k[1], True
    U = np.dtype("u%d" % np.dtype(name).itemsize).type
    return U(0), U(np.iinfo(U).max), False


def step_keys(K, name, method):
    "the predecessor (dilation) or successor (erosion) of every key, saturating at the ends of the order without NaN"
    low, high, has_nan = ends(name)
    top = ones_of(K)
    one = K.dtype.type(1)
    if method == "dilation":
        out = np.where(K <= low, K, K - one)
        return np.where(K == top, high, out).astype(K.dtype) if has_nan else out.astype(K.dtype)
    out = np.where(K >= high, K, K + one)
    return np.where(K == top, top, out).astype(K.dtype) if has_nan else out.astype(K.dtype)


def round_bfloat16(d):
    "float64 -> the uint16 bit patterns of bfloat16, rounded once to nearest even (8 significant bits, exponents as float32)"
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(all="ignore"):
        _, e = np.frexp(d)
        q = np.ldexp(1.0, np.maximum(e, -125) - 8)
        r = np.where(np.isfinite(d), np.rint(d / q) * q, d)
        r = np.where(np.abs(r) >= 2.0 ** 128, np.copysign(np.inf, r), r)
        f = r.astype(np.float32)
    assert np.all((f.astype(np.float64) == r) | np.isnan(r))
    return (np.ascontiguousarray(f).view(np.uint32) >> 16).astype(np.uint16)


def shift_keys(A, name, h, method):
    "the keys of mask - h (dilation) or mask + h (erosion): integers saturate, floats are computed in float64 and rounded once"
    assert np.isfinite(h) and h > 0
    sign = -1.0 if method == "dilation" else 1.0
    if name not in R.FLOATS:
        assert float(h) == int(h)
        info = np.iinfo(A.dtype)
        hh = min(int(h), 1 << 20)
        return R.key(np.clip(A.astype(np.int64) + int(sign) * hh, info.min, info.max).astype(A.dtype))
    if name == "bfloat16":
        v = (A.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        return R.key(round_bfloat16(v + sign * float(h)), "bfloat16")
    with np.errstate(all="ignore"):
        return R.key((A.astype(np.float64) + sign * float(h)).astype(A.dtype))


def rim_of(shape, faces):
    "the samples on the faces named by the bits: 0: i = 0, 1: i = n0-1, 2: j = 0, 3: j = n1-1, 4: k = 0, 5: k = n2-1"
    assert 1 <= faces <= 63
    on = np.zeros(shape, dtype=bool)
    for axis in range(3):
        for side in range(2):
            if faces >> (2 * axis + side) & 1:
                idx = [slice(None)] * 3
                idx[axis] = -1 if side else 0
                on[tuple(idx)] = True
    return on


def reconstruct(mask, marker="step", h=0.0, faces=ALL_FACES, method="dilation", connectivity=1, out_kind="values", dtype=None):
    """cx_grid_reconstruct3d of a 3-D mask -> (the result, n_changed, n_clamped).  marker: "shift", "step", "rim" or the marker array;
    dtype='bfloat16': the arrays hold uint16 bit patterns.  out_kind "values": the samples' type; "changed": uint8"""
    A = np.ascontiguousarray(mask)
    assert A.ndim == 3 and method in METHODS and out_kind in ("values", "changed")
    name = R.type_name(A, dtype)
    K = R.key(A, dtype)
    top = ones_of(K)
    flip = top if method == "erosion" else K.dtype.type(0)
    if isinstance(marker, str):
        if marker == "shift":
            G = shift_keys(A, name, h, method)
        elif marker == "step":
            G = step_keys(K, name, method)
        else:
            assert marker == "rim"
            G = np.where(rim_of(A.shape, faces), K, flip).astype(K.dtype)
    else:
        B = np.ascontiguousarray(marker)
        assert B.shape == A.shape and B.dtype == A.dtype
        G = R.key(B, dtype)
    W, GW = K ^ flip, G ^ flip      # the working keys: erosion is dilation of the complement
    n_clamped = int((GW > W).sum())
    GW = np.minimum(GW, W)
    RW = iterate(GW, W, connectivity)
    changed = RW != W
    n_changed = int(changed.sum())
    if out_kind == "values":
        return R.unkey(RW ^ flip, name), n_changed, n_clamped
    if isinstance(marker, str) and marker == "step" and name not in R.FLOATS and not (GW != W).any():
        changed = np.ones(A.shape, dtype=bool)      # every sample the extreme of the type: no predecessor, one regional extremum
    return changed.astype(np.uint8), n_changed, n_clamped
