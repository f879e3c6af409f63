"""float64 numpy restatement of the curvature definition in include/contourist_hip.h ("vertex attributes") and DESIGN.md 9i:
numpy.gradient for the gradient, second differences around the clamped centre for the Hessian, the same formulae.  Shared by
tests/test_curvature_host.py (CPU) and tests/test_gpu_curvature.py."""
import numpy as np

_E = np.eye(3, dtype=np.int64)


def gradient(A64):
    "numpy.gradient with its defaults: central difference inside, one-sided first difference on the rim; (n0, n1, n2, 3)"
    return np.stack(np.gradient(A64), axis=-1)


def hessian_at(A64, P):
    """H (m,3,3) at the lattice points P (m,3): second differences at the centre c = clamp(p, 1, n-2) per axis, in the
    definition's order of evaluation, and per entry (m,3,3) the sum of the absolute values of its two inner first differences, a
    mixed entry weighted by 0.25 (D of the bounds is the sum over all nine places, so a mixed entry counts twice)"""
    n = np.array(A64.shape, dtype=np.int64)
    assert np.all(n >= 3), "every axis needs 3 samples"
    C = np.clip(np.asarray(P, dtype=np.int64), 1, n - 2)

    def s(Q):
        return A64[Q[:, 0], Q[:, 1], Q[:, 2]]
    H = np.zeros((len(C), 3, 3))
    Dij = np.zeros((len(C), 3, 3))
    fc = s(C)
    for a in range(3):
        d1, d2 = s(C + _E[a]) - fc, fc - s(C - _E[a])
        H[:, a, a] = d1 - d2
        Dij[:, a, a] = np.abs(d1) + np.abs(d2)
        for b in range(a + 1, 3):
            d1 = s(C + _E[a] + _E[b]) - s(C + _E[a] - _E[b])
            d2 = s(C - _E[a] + _E[b]) - s(C - _E[a] - _E[b])
            H[:, a, b] = H[:, b, a] = (d1 - d2) * 0.25
            Dij[:, a, b] = Dij[:, b, a] = 0.25 * (np.abs(d1) + np.abs(d2))
    return H, Dij


def adjugate(H):
    "adj(H) of symmetric 3x3 matrices (m,3,3)"
    A = np.empty_like(H)
    A[:, 0, 0] = H[:, 1, 1] * H[:, 2, 2] - H[:, 1, 2] * H[:, 1, 2]
    A[:, 1, 1] = H[:, 0, 0] * H[:, 2, 2] - H[:, 0, 2] * H[:, 0, 2]
    A[:, 2, 2] = H[:, 0, 0] * H[:, 1, 1] - H[:, 0, 1] * H[:, 0, 1]
    A[:, 0, 1] = A[:, 1, 0] = H[:, 0, 2] * H[:, 1, 2] - H[:, 0, 1] * H[:, 2, 2]
    A[:, 0, 2] = A[:, 2, 0] = H[:, 0, 1] * H[:, 1, 2] - H[:, 0, 2] * H[:, 1, 1]
    A[:, 1, 2] = A[:, 2, 1] = H[:, 0, 1] * H[:, 0, 2] - H[:, 0, 0] * H[:, 1, 2]
    return A


def curvature(A64, a, b, r, delta=None, G=None):
    """the definition at the crossings of the edges a -> b (m,3 lattice points each) at fractions r (m,):
    dict(mean, gauss, k1, k2, g (|g|), n (m,3), Gs, D).  Gs = |G(a)|_1 + |G(b)|_1 and D = the sum over both end points of the
    inner first differences of H (hessian_at), both in the units of g and H (divided by delta like them).
    G: gradient(A64) when the caller has it already."""
    A64 = np.asarray(A64, dtype=np.float64)
    a, b = np.asarray(a, dtype=np.int64).reshape(-1, 3), np.asarray(b, dtype=np.int64).reshape(-1, 3)
    r = np.asarray(r, dtype=np.float64).reshape(-1)
    if G is None:
        G = gradient(A64)
    Ga, Gb = G[tuple(a.T)], G[tuple(b.T)]
    Ha, Da = hessian_at(A64, a)
    Hb, Db = hessian_at(A64, b)
    g = Ga + r[:, None] * (Gb - Ga)
    H = Ha + r[:, None, None] * (Hb - Ha)
    Gs3, D33 = np.abs(Ga) + np.abs(Gb), Da + Db
    if delta is not None:
        d = np.asarray(delta, dtype=np.float64).reshape(3)
        g, Gs3 = g / d, Gs3 / d
        H, D33 = H / (d[:, None] * d[None, :]), D33 / (d[:, None] * d[None, :])
    glen = np.sqrt((g * g).sum(axis=1))
    nz = glen > 0
    safe = np.where(nz, glen, 1.0)
    n = np.where(nz[:, None], g / safe[:, None], 0.0)
    nHn = np.einsum("mi,mij,mj->m", n, H, n)
    mean = (np.trace(H, axis1=1, axis2=2) - nHn) / (2.0 * safe)
    gauss = np.einsum("mi,mij,mj->m", n, adjugate(H), n) / safe ** 2
    root = np.sqrt(np.maximum(mean * mean - gauss, 0.0))
    k1, k2 = mean + root, mean - root
    for x in (mean, gauss, k1, k2):
        x[~nz] = 0.0
    return dict(mean=mean, gauss=gauss, k1=k1, k2=k2, g=glen, n=n, Gs=Gs3.sum(axis=1), D=D33.sum(axis=(1, 2)))


def bounds(ref, eps, C):
    """the three error bounds of the issue for a result of `curvature`: bm for mean, bk for gauss, and for k1, k2
    bm + sqrt(2 |mean| bm + bm^2 + bk) (|sqrt(x+e) - sqrt(x)| <= sqrt|e|).  Rows with |g| == 0 get 0: four zeros are asked for."""
    g = np.where(ref["g"] > 0, ref["g"], 1.0)
    bm = C * eps * (ref["D"] / g) * (ref["Gs"] / g)
    bk = C * eps * (ref["D"] / g) ** 2 * (ref["Gs"] / g)
    bp = bm + np.sqrt(2.0 * np.abs(ref["mean"]) * bm + bm * bm + bk)
    zero = ref["g"] == 0
    return np.where(zero, 0.0, bm), np.where(zero, 0.0, bk), np.where(zero, 0.0, bp)


def edge_crossings(A64, value):
    """every crossing of the isovalue on the 7 edge directions the march uses (d = 1..7, 4 di + 2 dj + dk), found as the march
    finds them ((f < value) differs at the two ends): a, b (m,3) and the float64 fraction r from a"""
    A64 = np.asarray(A64, dtype=np.float64)
    n = np.array(A64.shape)
    As, Bs, Rs = [], [], []
    for d in range(1, 8):
        step = np.array([(d >> 2) & 1, (d >> 1) & 1, d & 1])
        I = np.stack(np.meshgrid(*[np.arange(m - s) for m, s in zip(n, step)], indexing="ij"), axis=-1).reshape(-1, 3)
        fa, fb = A64[tuple(I.T)], A64[tuple((I + step).T)]
        m = (fa < value) != (fb < value)
        As.append(I[m]); Bs.append(I[m] + step); Rs.append((value - fa[m]) / (fb[m] - fa[m]))
    return np.concatenate(As), np.concatenate(Bs), np.concatenate(Rs)


# ---- fields of the tests ----------------------------------------------------------------------------------------------------
SPHERE_R, SPHERE_N = 7.3, 24
SPHERE_OFFSET = (0.13, 0.34, -0.04)          # the centre is off the lattice on every axis
TORUS_R, TORUS_r = 11.0, 4.5

# Relative error of the reference itself on the 24^3 quadratic sphere (R = 7.3, centre offset SPHERE_OFFSET), over all
# 2976 crossings of the 7 edge directions: 0.00712 for mean, k1 and k2, 0.01428 for gauss (crossings on axis edges alone: 0.0024 and
# 0.0047).  The asserted tolerance is four times the measurement, because another diagonal mix may shift it.
SPHERE_MEAN_RTOL = 4 * 0.00712
SPHERE_GAUSS_RTOL = 4 * 0.01428
# The extremes of gauss on the torus (R = 11, r = 4.5) in 40^3, 8682 crossings: -0.036222 and +0.014623 where the exact values are
# -1/(r (R - r)) = -0.034188 and 1/(r (R + r)) = +0.014337: 0.0595 and 0.0200 relative; again four times that.
TORUS_MIN_RTOL = 4 * 0.0595
TORUS_MAX_RTOL = 4 * 0.0200


def _axes(shape, offset):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) - (n - 1) / 2.0 + o for n, o in zip(shape, offset)], indexing="ij")


def quadratic_sphere(n=SPHERE_N, R=SPHERE_R, offset=SPHERE_OFFSET, centres=None, shape=None):
    """x^2 + y^2 + z^2 - R^2 as fp32 samples (isovalue 0, grows outwards); centres: several spheres, the minimum of their
    fields (each zero set is one sphere while they stay apart)"""
    shape = (n,) * 3 if shape is None else shape
    X, Y, Z = _axes(shape, offset)
    if centres is None:
        centres = [(0.0, 0.0, 0.0)]
    F = np.minimum.reduce([(X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2 - R * R for c in centres])
    return F.astype(np.float32)


def torus(shape=(40, 40, 20), R=TORUS_R, r=TORUS_r, offset=SPHERE_OFFSET):
    "(sqrt(x^2 + y^2) - R)^2 + z^2 - r^2 as fp32 samples (isovalue 0): Gaussian curvature from -1/(r (R-r)) to 1/(r (R+r))"
    X, Y, Z = _axes(shape, offset)
    return ((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z - r * r).astype(np.float32)


def double_torus(shape=(48, 32, 16), offset=SPHERE_OFFSET, c=9.0, R=6.0, r=2.6):
    """two tori side by side along the first axis, blended smoothly where their tubes meet: a closed surface of genus 2
    (f = t1 * t2 - e with t_i the torus fields; its zero set rounds off the union of the two tubes)"""
    X, Y, Z = _axes(shape, offset)
    t1 = (np.sqrt((X - c) ** 2 + Y * Y) - R) ** 2 + Z * Z - r * r
    t2 = (np.sqrt((X + c) ** 2 + Y * Y) - R) ** 2 + Z * Z - r * r
    return (t1 * t2 - 12.0).astype(np.float32)


def gauss_bonnet_fields():
    "name -> (fp32 samples, Euler numbers of the components); isovalue 0 everywhere.  Closed surfaces that grow outwards"
    return {
        "sphere": (quadratic_sphere(28, 9.3), [2]),
        "two_spheres": (quadratic_sphere(R=5.2, shape=(36, 20, 20), centres=[(-8.5, 0.0, 0.0), (8.5, 0.3, -0.2)]), [2, 2]),
        "torus": (torus(), [0]),
        "double_torus": (double_torus(), [-2]),
    }


def vertex_areas(points, triangles):
    "one third of the incident triangle areas per vertex"
    P, T = np.asarray(points, dtype=np.float64), np.asarray(triangles, dtype=np.int64)
    area = 0.5 * np.linalg.norm(np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]), axis=1)
    out = np.zeros(len(P))
    for c in range(3):
        np.add.at(out, T[:, c], area / 3.0)
    return out
