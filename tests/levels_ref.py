"""numpy restatement of include/contourist_hip.h, section "choosing isovalues": the order statistics of cx_samples_select (np.sort of the
fp32 values, and the order-preserving keys the kernels select on) and the per-level size curve of cx_level_spectrum3d -- once in the
difference-array form the kernel uses, once as a brute-force classifier per level.  Not imported by product code."""
import numpy as np

# tet vertex -> cube corner (csrc/cx_tables.h: CX_TET_CORNERS_INIT), corner c = 4 di + 2 dj + dk
TET_CORNERS = ((0, 7, 1, 3), (0, 7, 3, 2), (0, 7, 2, 6), (0, 7, 6, 4), (0, 7, 4, 5), (0, 7, 5, 1))
KEYS = ("n_cells", "n_vertices", "n_triangles", "n_near")


# ---- select ----------------------------------------------------------------------------------------------------------------------------
def as_f32(x):
    "the samples as the fp32 values the kernels order"
    return np.asarray(x).astype(np.float32)


def select(x, ranks):
    "(values, n_nan): np.sort order of the fp32 values"
    f = as_f32(x).reshape(-1)
    return np.sort(f)[np.asarray(ranks, dtype=np.int64)].astype(np.float64), int(np.isnan(f).sum())


def special_field():
    "fp32 noise with NaN of both signs and payloads, +-inf, +-0, the smallest and largest denormals and normals of both signs, each twice"
    rng = np.random.RandomState(3)
    x = rng.standard_normal(4000).astype(np.float32)
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001,
                     0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF], dtype=np.uint32).view(np.float32)
    return np.concatenate([x, bits, bits])


def key_f32(x):
    "the 32-bit keys of fp32 values: sign flip for non-negative values, full inversion for negative ones, NaN on top, -0.0 as +0.0"
    u = np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32).copy()
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    u[u == np.uint32(0x80000000)] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    k = np.where(neg, ~u, u | np.uint32(0x80000000))
    k[nan] = np.uint32(0xFFFFFFFF)
    return k


def percentile_values(samples, breakpoints):
    "multiple_2d_contour.py:84-98 on the samples as float64"
    ordered = np.sort(np.asarray(samples, dtype=np.float64), axis=None)
    stride = int(ordered.size / breakpoints)
    return list(ordered[stride::stride])


def linear_values(samples, breakpoints):
    "multiple_2d_contour.py:100-108"
    s = np.asarray(samples, dtype=np.float64)
    step = (s.max() - s.min()) * (1.0 / breakpoints)
    return [step * k for k in range(1, breakpoints)]


# ---- the march's value parameters (csrc/cx_api.hip: cx_fill_value_params) --------------------------------------------------------------
def value_params(value):
    "(vcmp, near_abs) as fp32"
    value = float(value)
    t = np.float32(value)
    if float(t) < value:
        t = np.nextafter(t, np.float32(np.inf))
    if t == 0:
        t = np.float32(-0.0)
    near = np.nextafter(np.float32(2.2e-5 * abs(value) + 4e-8), np.float32(np.inf))
    return np.float32(t), np.float32(near)


def _corner(A, d):
    "the samples at corner d of every cell"
    n0, n1, n2 = A.shape
    di, dj, dk = (d >> 2) & 1, (d >> 1) & 1, d & 1
    return A[di:n0 - 1 + di, dj:n1 - 1 + dj, dk:n2 - 1 + dk]


def _forward(A, d):
    "(lattice points that have the forward neighbour d inside the array, those neighbours)"
    n0, n1, n2 = A.shape
    di, dj, dk = (d >> 2) & 1, (d >> 1) & 1, d & 1
    return A[:n0 - di, :n1 - dj, :n2 - dk], A[di:, dj:, dk:]


# ---- brute force: one level at a time ---------------------------------------------------------------------------------------------------
def spectrum_one(A, value):
    "(n_cells, n_vertices, n_triangles, n_near) of one value, by classifying every cell, edge and tetrahedron"
    f = as_f32(A)
    vcmp, near = value_params(value)
    with np.errstate(invalid="ignore"):
        low = f < vcmp                       # NaN: never low
        n_near = int((np.abs(f - vcmp) <= near).sum())
    n_vertices = 0
    for d in range(1, 8):
        a, b = _forward(low, d)
        n_vertices += int((a != b).sum())
    corners = [_corner(low, d) for d in range(8)]
    nlow = sum(c.astype(np.int32) for c in corners)
    n_cells = int(((nlow > 0) & (nlow < 8)).sum())
    n_triangles = 0
    for tet in TET_CORNERS:
        m = sum(corners[c].astype(np.int32) for c in tet)
        n_triangles += int(((m == 1) | (m == 3)).sum()) + 2 * int((m == 2).sum())
    return n_cells, n_vertices, n_triangles, n_near


def spectrum_brute(A, values):
    out = np.array([spectrum_one(A, v) for v in values], dtype=np.int64).reshape(-1, 4)
    return {k: out[:, n].copy() for n, k in enumerate(KEYS)}


# ---- the difference-array form: all levels in one pass ------------------------------------------------------------------------------------
def spectrum(A, values):
    """dict of four int64 arrays in the order of `values`.  With the thresholds sorted, c(f) = thresholds <= f (K for a NaN); level s of
    the sorted order sees a sample low iff s >= c(f).  An edge adds +1 at the smaller c of its ends and -1 at the larger, a cell at the
    min and max of its 8, a tetrahedron with sorted c1..c4 adds +1, +1, -1, -1; the counts are prefix sums.  n_near: per level the
    samples between two fp32 bounds, the ends of its screen on the fp32 number line."""
    f = as_f32(A)
    values = np.asarray(values, dtype=np.float64).reshape(-1)
    K = len(values)
    params = [value_params(v) for v in values]
    vcmp = np.array([p[0] for p in params], dtype=np.float32)
    order = np.argsort(vcmp, kind="stable")
    tab = vcmp[order]
    c = np.searchsorted(tab, f, side="right").astype(np.int64)
    c[np.isnan(f)] = K
    de, dc, dt = (np.zeros(K + 1, dtype=np.int64) for _ in range(3))
    for d in range(1, 8):
        a, b = _forward(c, d)
        np.add.at(de, np.minimum(a, b).ravel(), 1)
        np.add.at(de, np.maximum(a, b).ravel(), -1)
    corners = np.stack([_corner(c, d) for d in range(8)])
    np.add.at(dc, corners.min(axis=0).ravel(), 1)
    np.add.at(dc, corners.max(axis=0).ravel(), -1)
    for tet in TET_CORNERS:
        s = np.sort(np.stack([corners[k] for k in tet]), axis=0)
        for row, sign in zip(s, (1, 1, -1, -1)):
            np.add.at(dt, row.ravel(), sign)
    out = {k: np.zeros(K, dtype=np.int64) for k in KEYS}
    out["n_vertices"][order] = np.cumsum(de)[:K]
    out["n_cells"][order] = np.cumsum(dc)[:K]
    out["n_triangles"][order] = np.cumsum(dt)[:K]
    # the screens: all fp32 numbers by key, the first and last key inside each level's screen by bisection with the fp32 expression
    keys = np.sort(key_f32(f))
    for l in range(K):
        lo, hi = screen_bounds(vcmp[l], params[l][1])
        out["n_near"][l] = int(np.searchsorted(keys, hi, side="right") - np.searchsorted(keys, lo, side="left"))
    return out


def unkey_f32(k):
    k = np.uint32(k)
    u = (k ^ np.uint32(0x80000000)) if (k & np.uint32(0x80000000)) else ~k
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def _inside(key, vcmp, near):
    with np.errstate(invalid="ignore", over="ignore"):
        return bool(np.abs(np.float32(unkey_f32(key) - vcmp)) <= near)


def screen_bounds(vcmp, near):
    "(first key, last key) of the fp32 numbers f with fabsf(f - vcmp) <= near_abs"
    kv = int(key_f32(vcmp)[0])
    a, b = 0x007FFFFF, kv
    while a < b:
        m = (a + b) // 2
        if _inside(m, vcmp, near):
            b = m
        else:
            a = m + 1
    lo = a
    a, b = kv, 0xFF800000
    while a < b:
        m = (a + b + 1) // 2
        if _inside(m, vcmp, near):
            a = m
        else:
            b = m - 1
    return lo, a
