"""Host side of the vertex curvature: the declarations, the Python methods, and the numpy reference
tests/curvature_ref.py on fields whose curvature is known.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import curvature_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "contourist_hip.h")
CALLS = ["cx_level0_curvature", "cx_level0_curvature_download", "cx_level1_curvature", "cx_level1_curvature_download"]

SPHERE_MEAN_RTOL, SPHERE_GAUSS_RTOL = cr.SPHERE_MEAN_RTOL, cr.SPHERE_GAUSS_RTOL
TORUS_MIN_RTOL, TORUS_MAX_RTOL = cr.TORUS_MIN_RTOL, cr.TORUS_MAX_RTOL


def test_declarations_present():
    from contourist_amd import _ffi
    text = open(HEADER).read()
    for name in CALLS:
        assert name in _ffi.SYMBOLS, name
        assert re.search(r"\bint %s\(cx_ctx\* ctx, const double\* delta3, " % name, text), name
    L = _ffi.load()
    vp = ctypes.c_void_p
    for name in CALLS:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == ([vp, vp, vp] if name.endswith("_download") else [vp, vp, ctypes.POINTER(vp)]), name


def test_python_methods_exist():
    from contourist_amd import _ffi, tetrahedral
    for method in ("level0_curvature", "level1_curvature"):
        assert callable(getattr(_ffi.Context, method))
    for method in ("level0_curvature", "vertex_curvature"):
        assert callable(getattr(tetrahedral.GridContour3d, method))
    assert callable(tetrahedral.Delta3DContour.vertex_curvature)
    assert callable(tetrahedral.LevelResult.vertex_curvature)


def test_reference_on_the_quadratic_sphere():
    """mean = k1 = k2 = 1/R and gauss = 1/R^2 to SPHERE_MEAN_RTOL / SPHERE_GAUSS_RTOL (four times the measured 0.00712 / 0.01428),
    positive because the field grows outwards, at every crossing of the 24^3 sphere"""
    R = cr.SPHERE_R
    A = cr.quadratic_sphere()
    a, b, r = cr.edge_crossings(A, 0.0)
    c = cr.curvature(A, a, b, r)
    assert len(r) > 2000 and np.all(c["g"] > 0)
    worst = {k: float(np.abs(c[k] * R - 1).max()) for k in ("mean", "k1", "k2")}
    worst["gauss"] = float(np.abs(c["gauss"] * R * R - 1).max())
    print("sphere, crossings", len(r), "worst relative errors", worst)
    assert worst["mean"] <= SPHERE_MEAN_RTOL and worst["k1"] <= SPHERE_MEAN_RTOL and worst["k2"] <= SPHERE_MEAN_RTOL
    assert worst["gauss"] <= SPHERE_GAUSS_RTOL
    assert np.all(c["k1"] >= c["k2"])
    # the same surface from the field that grows inwards: the sign follows the gradient
    c2 = cr.curvature(-A.astype(np.float64), a, b, r)
    assert np.allclose(c2["mean"], -c["mean"], rtol=0, atol=1e-15) and np.allclose(c2["gauss"], c["gauss"], rtol=0, atol=1e-15)
    assert np.allclose(c2["k1"], -c["k2"], rtol=0, atol=1e-15) and np.allclose(c2["k2"], -c["k1"], rtol=0, atol=1e-15)


def test_reference_in_world_units():
    """a sphere of world radius R sampled at spacing delta per axis: 1/R with delta handed over.  The bound is analytic: for
    |x|^2 - R^2 the second differences and the central first differences are exact and the gradient is linear, so the lerped g and H
    are those of the point the linear interpolation puts the crossing at.  On an edge of world length L that point has
    f = -s (L - s) >= -L^2 / 4, i.e. radius rho with rho^2 >= R^2 - L^2 / 4, and mean = 1 / rho, gauss = 1 / rho^2.  L^2 <= 5.25 for
    delta = (0.5, 1, 2); 1e-3 on top for the fp32 rounding of the samples (2^-24 * 600 per sample against second differences of 0.5)."""
    R, delta = cr.SPHERE_R, np.array([0.5, 1.0, 2.0])
    shape = (48, 24, 12)
    X, Y, Z = [g * d for g, d in zip(cr._axes(shape, cr.SPHERE_OFFSET), delta)]
    A = (X * X + Y * Y + Z * Z - R * R).astype(np.float32)
    a, b, r = cr.edge_crossings(A, 0.0)
    c = cr.curvature(A, a, b, r, delta=delta)
    inside = np.all((a >= 1) & (b <= np.array(shape) - 2), axis=1)      # (central differences at both ends)
    assert inside.sum() > 2000
    shrink = 1.0 - float((delta ** 2).sum()) / (4 * R * R)
    em, eg = float(np.abs(c["mean"] * R - 1)[inside].max()), float(np.abs(c["gauss"] * R * R - 1)[inside].max())
    print("world sphere, crossings", int(inside.sum()), "worst", em, eg, "bounds", shrink ** -0.5 - 1, 1 / shrink - 1)
    assert em <= shrink ** -0.5 - 1 + 1e-3 and eg <= 1 / shrink - 1 + 1e-3
    assert np.all(c["mean"][inside] * R >= 1 - 1e-3)                     # the interpolated point is never outside the sphere


def test_reference_on_the_torus_extremes():
    "the extremes of gauss on the torus to TORUS_MIN_RTOL / TORUS_MAX_RTOL (four times the measured 0.0595 / 0.0200)"
    R, r0 = cr.TORUS_R, cr.TORUS_r
    A = cr.torus((40, 40, 40))
    a, b, r = cr.edge_crossings(A, 0.0)
    c = cr.curvature(A, a, b, r)
    lo, hi = float(c["gauss"].min()), float(c["gauss"].max())
    exact_lo, exact_hi = -1.0 / (r0 * (R - r0)), 1.0 / (r0 * (R + r0))
    print("torus, crossings", len(r), "gauss from", lo, "to", hi, "exact", exact_lo, exact_hi)
    assert abs(lo / exact_lo - 1) <= TORUS_MIN_RTOL and abs(hi / exact_hi - 1) <= TORUS_MAX_RTOL


def test_rim_takes_the_nearest_interior_hessian():
    "a sphere cut open by the array's rim: the crossings on the rim planes are as good as the others"
    n, R = 24, 8.3
    X, Y, Z = np.meshgrid(np.arange(n) + 0.13, np.arange(n) - 11.0, np.arange(n) - 11.0, indexing="ij")
    A = (X * X + Y * Y + Z * Z - R * R).astype(np.float32)
    a, b, r = cr.edge_crossings(A, 0.0)
    on_rim = (a[:, 0] == 0) & (b[:, 0] == 0)
    assert on_rim.sum() > 50
    c = cr.curvature(A, a, b, r)
    assert np.abs(c["mean"][on_rim] * R - 1).max() <= SPHERE_MEAN_RTOL and np.abs(c["gauss"][on_rim] * R * R - 1).max() <= SPHERE_GAUSS_RTOL
    H, _D = cr.hessian_at(A.astype(np.float64), np.array([[0, 5, 5], [1, 5, 5], [23, 0, 23], [22, 1, 22]]))
    assert np.array_equal(H[0], H[1]) and np.array_equal(H[2], H[3])
    with pytest.raises(AssertionError):
        cr.hessian_at(np.zeros((6, 5, 2)), np.array([[0, 0, 0]]))


# ---- Gauss-Bonnet with the reference alone, on meshes of the oracle's march ---------------------------------------------------
def _components(nv, T):
    "label of every vertex: the smallest vertex index of its component"
    lab = np.arange(nv)
    while True:
        old = lab.copy()
        mn = np.minimum.reduce([lab[T[:, 0]], lab[T[:, 1]], lab[T[:, 2]]])
        for k in range(3):
            np.minimum.at(lab, T[:, k], mn)
        lab = lab[lab]
        if np.array_equal(old, lab):
            return lab


@pytest.mark.parametrize("name", ["sphere", "two_spheres", "torus", "double_torus"])
def test_gauss_bonnet_of_the_reference(name):
    """sum(gauss * vertex area) / 2 pi per component within 0.5 of the Euler number V - E + F (integrality: the nearest integer
    is then the right one), with curvature_ref at the vertices of the oracle's Level-0 mesh.  Measured: 1.998 (sphere), 1.994 and
    1.995 (two spheres), -0.010 (torus), -1.860 (double torus)."""
    from oracle import level0
    A, eulers = cr.gauss_bonnet_fields()[name]
    m = level0.march3d(A, 0.0)
    P = m["pairs"].astype(np.int64)
    lo, hi = np.minimum(P[:, :3], P[:, 3:]), np.maximum(P[:, :3], P[:, 3:])
    r = np.abs(m["xyz"] - lo).max(axis=1)                    # the fraction from the lexicographically smaller end
    c = cr.curvature(A, lo, hi, r)
    T = m["tris"]
    area = cr.vertex_areas(m["xyz"], T)
    lab = _components(len(lo), T)
    roots = np.unique(lab)
    assert len(roots) == len(eulers)
    for root, expect in zip(roots, eulers):
        vs = lab == root
        ts = T[vs[T[:, 0]]]
        edges = np.unique(np.sort(np.concatenate([ts[:, [0, 1]], ts[:, [1, 2]], ts[:, [2, 0]]]), axis=1), axis=0)
        chi = int(vs.sum()) - len(edges) + len(ts)
        total = float((c["gauss"][vs] * area[vs]).sum() / (2 * np.pi))
        print(name, "vertices", int(vs.sum()), "Euler number", chi, "integral / 2 pi", total)
        assert chi == expect
        assert abs(total - chi) < 0.5
