"""numpy restatement of cx_grid_resample3d (include/contourist_hip.h, "resampling through an affine map"), vectorised, in float64.

For output index (i0, i1, i2) the source coordinate on input axis a is c_a = ((offset[a] + M[a][0] i0) + M[a][1] i1) + M[a][2] i2, every
product and every sum a float64 operation of its own (numpy never fuses them).  Order 0 reads the sample at floor(c + 0.5) in the
input's own type; order 1 is the trilinear blend of the eight corners around floor(c), widened to float64, with
lerp(a, b, t) = a where t == 0 else a + t (b - a), reduced along input axis 2, then 1, then 0, and rounded to float32 once.
`src` is the filter's boundary rule (tests/filter_ref.py).  n_outside counts the outputs with some c_a < 0 or c_a > n_a - 1."""
import numpy as np

from filter_ref import MODES, src      # noqa: F401  (MODES: what the tests parametrise over)

LIMIT = float(1 << 20)      # the largest magnitude of a matrix or offset entry


def coordinates(matrix, offset, out_shape):
    "the three float64 arrays c_a of shape out_shape"
    M = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    i0, i1, i2 = np.meshgrid(*[np.arange(int(m), dtype=np.float64) for m in out_shape], indexing="ij")
    return [((off[a] + M[a, 0] * i0) + M[a, 1] * i1) + M[a, 2] * i2 for a in range(3)]


def count_outside(c, shape):
    out = np.zeros(c[0].shape, dtype=bool)
    for a in range(3):
        out |= (c[a] < 0.0) | (c[a] > np.float64(shape[a] - 1))
    return int(out.sum())


def widen(samples, dtype=None):
    "the samples as float64; dtype 'bfloat16': they are the uint16 bit patterns"
    a = np.asarray(samples)
    if dtype is not None and str(dtype).endswith("bfloat16"):
        assert a.dtype == np.uint16
        return (a.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def fill_of(cval, np_dtype, dtype=None):
    "cval in the samples' own type (order 0); it must be exact there"
    if dtype is not None and str(dtype).endswith("bfloat16"):
        b = np.asarray([cval], dtype=np.float32).view(np.uint32)[0]
        assert (b & 0xFFFF) == 0 and float(np.float32(cval)) == float(cval)
        return np.uint16(b >> 16)
    v = np.asarray([cval]).astype(np_dtype)[0]
    assert float(v) == float(cval), "cval is not exact in %s" % np.dtype(np_dtype).name
    return v


def lerp(a, b, t):
    with np.errstate(all="ignore"):
        return np.where(t == 0.0, a, a + t * (b - a))


def resample(samples, matrix, offset, out_shape, order=1, mode="nearest", cval=0.0, dtype=None):
    """-> (result, n_outside).  samples: 3-D; dtype="bfloat16": uint16 bit patterns of bfloat16 samples.  Order 0: the result has the
    samples' numpy type; order 1: float32."""
    A = np.ascontiguousarray(samples)
    assert A.ndim == 3 and order in (0, 1)
    n = A.shape
    c = coordinates(matrix, offset, out_shape)
    n_outside = count_outside(c, n)
    if order == 0:
        idx, outside = [], np.zeros(c[0].shape, dtype=bool)
        for a in range(3):
            j, o = src(np.floor(c[a] + 0.5).astype(np.int64), n[a], mode)
            idx.append(j)
            outside |= o
        out = A[idx[0], idx[1], idx[2]]
        if mode == "constant":
            out = np.where(outside, fill_of(cval, A.dtype, dtype), out).astype(A.dtype)
        return np.ascontiguousarray(out), n_outside
    W = widen(A, dtype)
    fill = np.float64(np.float32(cval))
    lo = [np.floor(c[a]) for a in range(3)]
    t = [c[a] - lo[a] for a in range(3)]
    lo = [x.astype(np.int64) for x in lo]
    corner = {}
    for d0 in (0, 1):
        j0, o0 = src(lo[0] + d0, n[0], mode)
        for d1 in (0, 1):
            j1, o1 = src(lo[1] + d1, n[1], mode)
            for d2 in (0, 1):
                j2, o2 = src(lo[2] + d2, n[2], mode)
                v = W[j0, j1, j2]
                corner[d0, d1, d2] = np.where(o0 | o1 | o2, fill, v) if mode == "constant" else v
    along2 = {(d0, d1): lerp(corner[d0, d1, 0], corner[d0, d1, 1], t[2]) for d0 in (0, 1) for d1 in (0, 1)}
    along1 = {d0: lerp(along2[d0, 0], along2[d0, 1], t[1]) for d0 in (0, 1)}
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(lerp(along1[0], along1[1], t[0]).astype(np.float32)), n_outside


def same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def same_bits_nan(got, want):
    "float32 results: the NaNs in the same places, the bits equal elsewhere"
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != np.float32 or want.dtype != np.float32:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


# ---- maps the tests share -------------------------------------------------------------------------------------------------------------
def rotation(axis, degrees):
    "3 x 3 rotation about a coordinate axis (0, 1, 2) or about a vector"
    th = np.deg2rad(float(degrees))
    if np.ndim(axis) == 0:
        u = np.zeros(3)
        u[int(axis)] = 1.0
    else:
        u = np.asarray(axis, dtype=np.float64)
        u = u / np.linalg.norm(u)
    K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def about_centre(M, in_shape, out_shape):
    "(matrix, offset) of the map that takes the output's centre to the input's centre with linear part M"
    M = np.asarray(M, dtype=np.float64)
    ci = (np.asarray(in_shape, dtype=np.float64) - 1.0) / 2.0
    co = (np.asarray(out_shape, dtype=np.float64) - 1.0) / 2.0
    return M, ci - M @ co
