"""CPU: the numpy oracles of the 4-D back half against the loop versions they restate, element for element.

oracle/postpass4d.collect_morph_triangles_np and oracle/morph_eval.SurfaceStream / surface_at_np exist so that the GPU tests can hold
config 4 (25 M morph triangles) to an oracle; the loop versions are the ones pinned to the reference (tests/test_oracle4d_vs_golden.py,
tests/test_oracle_viewer.py).  Here both run on every tests/golden4d fixture, on the reference's own morph triangles (mt_*), on small
random fields (some quantised, so that vertex times tie) and on random tetrahedra over a long time axis, and must agree exactly:
same dict, same arrays, same dtypes; surfaces with the same active triangles in the same order, the same first-use numbering and the
same points bit for bit -- at generic times, on vertex times, at both ends of the range and outside it."""
import os

import numpy as np
import pytest

from conftest import ROOT
from oracle import level0_4d, morph_eval, postpass4d

G4 = os.path.join(ROOT, "tests", "golden4d")


def fixtures():
    return sorted(f[:-4] for f in os.listdir(G4) if f.endswith(".npz")) if os.path.isdir(G4) else []


def same_morph(keys, xyzt, tets, chunk=4096):
    """both versions of the slicing; the numpy one in small chunks, so that triangles meet again across chunks"""
    L = postpass4d.collect_morph_triangles(keys, xyzt, tets)
    N = postpass4d.collect_morph_triangles_np(keys, xyzt, tets, chunk=chunk)
    assert sorted(L) == sorted(N)
    for k in L:
        assert L[k].dtype == N[k].dtype and L[k].shape == N[k].shape, (k, L[k].dtype, N[k].dtype, L[k].shape, N[k].shape)
        assert np.array_equal(L[k].view(np.uint64) if L[k].dtype == np.float64 else L[k],
                              N[k].view(np.uint64) if N[k].dtype == np.float64 else N[k]), k
    return L


def probe_times(P, rng, n_vertex_times=3):
    "generic times, times equal to vertex times, both ends of the range, outside it"
    tv = np.unique(np.asarray(P)[:, 3])
    lo, hi = float(tv[0]), float(tv[-1])
    out = [lo + f * (hi - lo) for f in (0.013, 0.503, 0.811)]
    out += [float(x) for x in rng.choice(tv, size=min(n_vertex_times, len(tv)), replace=False)]
    out += [lo, hi, lo - 1.0, hi + 0.5]
    return out


def same_surfaces(P, S, T, times):
    "surface_at (loops) == SurfaceStream.surface_at == surface_at_np; -> triangles over all times"
    a = morph_eval.triangle_intervals(P, S, T)
    b = morph_eval.triangle_intervals_np(P, S, T)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    stream = morph_eval.SurfaceStream(P, S, T)
    total = 0
    for n, t in enumerate(times):
        W = morph_eval.surface_at(P, S, T, t)
        N = stream.surface_at(t) if n else morph_eval.surface_at_np(P, S, T, t)
        assert np.array_equal(np.asarray(W["active"], dtype=np.int64), N["active"]), t
        assert np.array_equal(np.asarray(W["segment_ids"], dtype=np.int64), N["segment_ids"]), t
        assert W["faces"].dtype == N["faces"].dtype and np.array_equal(W["faces"], N["faces"]), t
        assert W["points"].shape == N["points"].shape and np.array_equal(W["points"].view(np.uint64), N["points"].view(np.uint64)), t
        total += len(N["faces"])
    return total


def post_steps(A, v):
    corner = np.array(A.shape) - 1
    O = level0_4d.march4d(A, v, diag_mode=1)
    ko = level0_4d.edge_keys4(O["pairs"], A.shape)
    W = postpass4d.find_tetrahedra_post(ko, O["xyzt"], O["tets"], corner)
    return ko, O, W


@pytest.mark.parametrize("name", fixtures())
def test_morph_triangles_np_on_the_fixtures(name):
    """every fixture: march (or the reference's Level-0 edges where the fixture holds no samples), post steps, slicing -- both
    versions equal; then the surfaces of the result at probe times"""
    G = np.load(os.path.join(G4, name + ".npz"))
    rng = np.random.RandomState(len(name))
    if "A" in G.files or name == "reference_test0_seeded":
        if "A" in G.files:
            A = G["A"]
        else:
            from oracle.make_goldens4d import test0_field
            g = np.arange(9, dtype=np.float64)
            A = test0_field(*np.meshgrid(g, g, g, g, indexing="ij")).astype(np.float32)
        ko, O, W = post_steps(A, float(G["value"]))
        M = same_morph(ko, W["xyzt"], W["tets"])
        same_morph(ko, O["xyzt"], O["tets"])                          # unbinned times as well
    else:
        # only the reference's edges and tetrahedra: every vertex at the midpoint of its lattice edge (half-integer times, many ties)
        P = G["l0_pairs"].astype(np.int64)
        P = P - np.tile(P.reshape(-1, 4).min(axis=0), 2)
        ko = level0_4d.edge_keys4(P, P.reshape(-1, 4).max(axis=0) + 1)
        xyzt = 0.5 * (P[:, :4] + P[:, 4:]).astype(np.float64)
        M = same_morph(ko, xyzt, G["l0_tets"])
    assert len(M["triangles"]) > 1000
    assert same_surfaces(M["points4d"], M["segments"], M["triangles"], probe_times(M["points4d"], rng)) > 0


@pytest.mark.parametrize("name", [n for n in fixtures() if "mt_points4d" in np.load(os.path.join(G4, n + ".npz")).files])
def test_surfaces_np_on_the_reference_morph_triangles(name):
    "the reference's own morph triangles (its numbering, its 4-segment splits, its orientation) through both viewer restatements"
    G = np.load(os.path.join(G4, name + ".npz"))
    P, S, T = G["mt_points4d"], G["mt_segments"], G["mt_triangles"]
    assert same_surfaces(P, S, T, probe_times(P, np.random.RandomState(7))) > 0


@pytest.mark.parametrize("seed,quantise", [(1, False), (2, False), (3, True), (4, True)])
def test_np_oracles_on_small_random_fields(seed, quantise):
    """10 x 9 x 8 x 12: a moving blob in noise; quantised fields take few sample values, so that crossings sit on lattice points
    and vertex times tie before binning as well as after"""
    rng = np.random.RandomState(seed)
    shape = (10, 9, 8, 12)
    X, Y, Z, T = np.meshgrid(*[np.linspace(0.0, 1.0, n) for n in shape], indexing="ij")
    A = np.exp(-(((X - 0.35 - 0.3 * T) ** 2 + (Y - 0.45) ** 2 + (Z - 0.5) ** 2) / (2 * 0.2 ** 2))) + 0.15 * rng.standard_normal(shape)
    if quantise:
        A = np.round(A * 8.0) / 8.0
    A = np.ascontiguousarray(A.astype(np.float32))
    ko, O, W = post_steps(A, 0.5)
    M = same_morph(ko, W["xyzt"], W["tets"], chunk=1000)
    same_morph(ko, O["xyzt"], O["tets"], chunk=1000)
    assert len(M["triangles"]) > 10000
    same_surfaces(M["points4d"], M["segments"], M["triangles"], probe_times(M["points4d"], rng, 2))


@pytest.mark.parametrize("seed", [5, 6])
def test_morph_triangles_np_on_random_tetrahedra_over_a_long_time_axis(seed):
    """random tetrahedra over random vertices on a time axis long enough that the t_eps filter (1e-7 of the range of ALL vertex
    times) removes triangles; two vertices no tetrahedron uses stretch that range; times on a coarse grid tie"""
    rng = np.random.RandomState(seed)
    nv, nt = 400, 3000
    xyzt = rng.uniform(0.0, 10.0, size=(nv, 4))
    xyzt[:, 3] = np.round(rng.uniform(0.0, 1.0e4, size=nv) / 3.0e-4) * 3.0e-4       # steps of 3e-4: gaps above and below 1e-4 ... t_eps
    xyzt[:nv // 2, 3] = np.round(xyzt[:nv // 2, 3] / 50.0) * 50.0 + rng.choice([0.0, 1e-3, 2e-5], size=nv // 2)
    xyzt[-2:, 3] = [-1.0e5, 2.0e5]                                                    # unused: t_eps = 1e-7 * 3e5 = 0.03
    keys = rng.permutation(10 * nv)[:nv].astype(np.int64)
    tets = np.array([rng.choice(nv - 2, size=4, replace=False) for _ in range(nt)], dtype=np.int64)
    tets[nt // 2:] = tets[: nt - nt // 2][:, [2, 0, 3, 1]]                            # the same tetrahedra again, listed otherwise
    L = same_morph(keys, xyzt, tets, chunk=777)
    used = np.unique(tets)
    t_eps_used = 1e-7 * (xyzt[used, 3].max() - xyzt[used, 3].min())
    dt = np.abs(np.diff(L["points4d"][L["segments"], 3], axis=1))
    assert len(L["triangles"]) > 1000 and dt.min() > 1e-7 * 3e5 > t_eps_used
    same_surfaces(L["points4d"], L["segments"], L["triangles"], probe_times(L["points4d"][:-2], rng, 6))


def test_triangle_intervals_np_errors_as_the_loop():
    """a segment running backwards in time is an error -- unless a segment without time extent comes first in the same triangle,
    which ends the loop's look at it (the triangle is just invalid); a triangle lives on [tr_min, tr_max)"""
    P = np.array([[0, 0, 0, 0.0], [1, 0, 0, 2.0], [0, 1, 0, 3.0], [0, 0, 1, 1.0], [1, 1, 0, 3.0]])
    S = np.array([[0, 1], [0, 2], [3, 1], [2, 4], [2, 3]])        # 0 -> 2, 0 -> 3, 1 -> 2, 3 -> 3 (no extent), 3 -> 1 (backwards)
    ok = np.array([[0, 1, 2]])                                      # lives on [1, 2)
    for tris, raises in ((ok, False), (np.array([[0, 1, 2], [3, 4, 0]]), False), (np.array([[0, 4, 1]]), True),
                         (np.array([[1, 3, 4], [0, 1, 2]]), False), (np.array([[0, 1, 2], [4, 3, 0]]), True)):
        if raises:
            for fn in (morph_eval.triangle_intervals, morph_eval.triangle_intervals_np):
                with pytest.raises(ValueError):
                    fn(P, S, tris)
        else:
            a, b = morph_eval.triangle_intervals(P, S, tris), morph_eval.triangle_intervals_np(P, S, tris)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[2].sum() == 1
    for t, n in ((0.5, 0), (1.0, 1), (1.5, 1), (2.0, 0)):
        W = morph_eval.surface_at(P, S, ok, t)
        N = morph_eval.surface_at_np(P, S, ok, t)
        assert len(W["faces"]) == len(N["faces"]) == n and np.array_equal(W["faces"], N["faces"])
        assert np.array_equal(W["points"].view(np.uint64), N["points"].view(np.uint64))
