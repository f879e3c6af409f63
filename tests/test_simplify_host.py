"""Host side of the simplification (cx_simplify.hip): properties of the numpy restatement tests/simplify_ref.py of the header's
section "simplification" on the Level-1 meshes of committed fixtures and on an analytic sphere, and the agreement of the Python
constants and declarations with the header text.  No GPU.

This file also vets the inputs of an idempotence check: applying the clustering twice with the same cell keeps counts and
triangles and moves no coordinate by more than 2^-q ONLY where no mean of the first pass rounds onto a cell face (the second pass
would then put it into the neighbouring cell).  _stable() decides that per input; the inputs checked are INPUTS x CELLS below, and
every one of them is asserted stable (so a fixture that stops being stable fails here instead of silently leaving the case)."""
import os
import re

import numpy as np
import pytest

import simplify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "contourist_hip.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
INPUTS = ["sphere32", "blobs27", "shells24", "noise24_v0", "analytic_sphere"]
CELLS = [1.5, 2.0, 4.0, (2.0, 3.0, 5.0)]


def _mesh(name):
    "-> (points, triangles, corner)"
    if name == "analytic_sphere":
        P, T = R.sphere_mesh()
        return P, T, (25, 25, 25)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["l1_grid_points"], z["l1_triangles"], tuple(int(n) - 1 for n in z["A"].shape)


def _stable(S, corner, cell):
    "every vertex of the result still lies in the cell of its cluster: a second pass leaves every cluster a single vertex"
    c = np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,))
    k = np.floor(S["points"] / c).astype(np.int64)
    return np.array_equal(k, S["cell_of_new"])


def _run(name, cell, by_component=True):
    P, T, corner = _mesh(name)
    tl, vl = R.vertex_labels(T, len(P))
    S = R.simplify(P, T, corner, cell, by_component, vlab=vl)
    cid, first, kcell = R.clusters(P, vl, corner, cell, by_component)
    S["cell_of_new"] = kcell[S["keys"].astype(np.int64)]
    return P, T, corner, vl, S, kcell


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("cell", CELLS, ids=str)
def test_members_share_cell_and_label_and_stay_within_a_cell(name, cell):
    P, T, corner, vl, S, kcell = _run(name, cell)
    c = np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,))
    cid = S["cluster"]
    assert np.all(cid[vl >= 0] >= 0) and np.all(cid[vl < 0] < 0)
    mem = cid >= 0
    f = S["first"][cid[mem]]
    assert np.array_equal(kcell[mem], kcell[f]) and np.array_equal(vl[mem], vl[f])    # members share cell and label
    assert np.all(np.diff(S["first"]) > 0) and np.array_equal(np.unique(f), S["first"])
    for i in range(0, S["n_clusters"], max(1, S["n_clusters"] // 64)):               # first member = smallest old index
        assert int(np.nonzero(cid == i)[0][0]) == int(S["first"][i])
    m = S["map"] >= 0
    d = np.abs(P[m] - S["points"][S["map"][m]])
    assert np.all(d <= c), d.max(axis=0)                                              # every old vertex within cell_a of its new vertex
    assert S["clamped"] == 0 and S["q"] == R.q_of(corner)
    t = S["triangles"]
    assert len(t) <= S["n_distinct"] and (len(t) == 0 or (t.min() == 0 and t.max() == len(S["points"]) - 1))
    assert len(np.unique(np.sort(t, axis=1), axis=0)) == len(t)                     # no vertex set twice
    assert np.all(np.diff(S["old_triangle"]) > 0)                                    # relative order kept
    # winding kept: every surviving row is its old row through the map
    assert np.array_equal(t, S["map"][np.asarray(T)[S["old_triangle"]]])


@pytest.mark.parametrize("name", INPUTS)
@pytest.mark.parametrize("cell", CELLS, ids=str)
def test_twice_is_once(name, cell):
    "derived: a cluster of one member has its own fixed-point rounding as its mean, |x - rint(x 2^q) 2^-q| <= 2^-(q+1)"
    P, T, corner, vl, S, kcell = _run(name, cell)
    assert _stable(S, corner, cell), "a mean of %s at cell %s rounds onto a cell face: take this input out of INPUTS" % (name, cell)
    S2 = R.simplify(S["points"], S["triangles"], corner, cell)
    assert len(S2["points"]) == len(S["points"]) and S2["n_clusters"] == len(S["points"])
    assert np.array_equal(S2["triangles"], S["triangles"])
    assert np.all(np.abs(S2["points"] - S["points"]) <= 2.0 ** -S["q"])
    assert np.array_equal(S2["map"], np.arange(len(S["points"])))


def _two_sheets():
    "two parallel sheets half a cell (of 2) apart, both inside the cells z in [10, 12)"
    n = 12
    I, J = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, d], axis=1), np.stack([a, d, c], axis=1)])
    sheet = lambda z: np.stack([I.ravel() + 0.37, J.ravel() + 0.41, np.full(n * n, z)], axis=1)
    return np.concatenate([sheet(10.2), sheet(11.2)]), np.concatenate([tri, tri + n * n]).astype(np.int32), (16, 16, 16)


def test_components_merge_only_across():
    P, T, corner = _two_sheets()
    tl, vl = R.vertex_labels(T, len(P))
    assert tl.max() == 1
    S = R.simplify(P, T, corner, 2.0, True, vlab=vl)
    lab_of_new = vl[S["keys"].astype(np.int64)]
    assert np.array_equal(vl[S["map"] >= 0], lab_of_new[S["map"][S["map"] >= 0]])      # no cluster holds both sheets
    assert R.vertex_labels(S["triangles"], len(S["points"]))[0].max() == 1            # still two components
    assert set(np.round(S["points"][:, 2], 6)) == {10.2, 11.2}
    A = R.simplify(P, T, corner, 2.0, False, vlab=vl)
    assert A["n_clusters"] * 2 == S["n_clusters"]
    assert np.allclose(A["points"][:, 2], 10.7)                                      # the sheets fused
    assert R.vertex_labels(A["triangles"], len(A["points"]))[0].max() == 0            # and the components merged
    assert len(A["triangles"]) * 2 == len(S["triangles"])                            # the second sheet's triangles were duplicates


def test_exact_mean_is_order_independent_and_rounded_once():
    rng = np.random.default_rng(11)
    P = rng.uniform(3.0, 5.0, size=(3000, 3))
    P[:, 0] = rng.uniform(4.0, 4.999, size=3000)
    corner = (40, 40, 40)
    vl = np.zeros(len(P), dtype=np.int32)
    cid, first, _k = R.clusters(P, vl, corner, 8.0)
    assert len(first) == 1 and first[0] == 0
    q = R.q_of(corner)
    assert q == 52 - 6
    a, _c = R.exact_means(P, cid, 1, corner, q)
    perm = rng.permutation(len(P))
    b, _c = R.exact_means(P[perm], cid, 1, corner, q)
    assert a.tobytes() == b.tobytes()
    from fractions import Fraction
    for k in range(3):
        exact = sum(Fraction(int(x)) for x in np.rint(P[:, k] * 2.0 ** q).astype(np.int64))
        assert a[0, k] == float(exact) / 3000.0 * 2.0 ** -q
        assert abs(Fraction(a[0, k]) - exact / 3000 / 2 ** q) <= Fraction(1, 2 ** 50)


def test_cells_limit_and_clamp():
    assert R.admissible((511, 511, 511), (0.5, 0.5, 0.5)) and not R.admissible((511, 511, 511), (0.25, 0.25, 0.25))
    kmin, kn = R.cell_box((10, 10, 10), (4.0, 4.0, 4.0))
    assert kmin.tolist() == [-1, -1, -1] and kn.tolist() == [4, 4, 4]                 # cells -1 .. 2: floor(-1/4) .. floor(11/4)
    P = np.array([[-0.5, 3.0, 12.5], [-0.25, 3.5, 11.5]])
    cid, first, k = R.clusters(P, np.zeros(2, dtype=np.int32), (10, 10, 10), 4.0)
    assert k.tolist() == [[-1, 0, 2], [-1, 0, 2]] and cid.tolist() == [0, 0]          # floor, not truncation; outside: the nearest cell
    pos, clamped = R.exact_means(P, cid, 1, (10, 10, 10), R.q_of((10, 10, 10)))
    assert clamped == 2 and pos[0].tolist() == [-0.375, 3.25, 11.0]


def test_constants_and_declarations_agree_with_the_header():
    from contourist_amd import _ffi, tetrahedral
    text = open(HEADER).read()
    sec = text[text.index("---- simplification"):]
    sec = sec[:sec.index("cx_level1_simplify_map_download(") + 200]
    flags = dict(re.findall(r"#define (CX_SIMPLIFY_\w+)\s+(\d+)u", sec))
    assert flags == {"CX_SIMPLIFY_NO_CLEAN": "1", "CX_SIMPLIFY_ACROSS_COMPONENTS": "2", "CX_SIMPLIFY_COUNT_ONLY": "4", "CX_SIMPLIFY_NORMALS": "8"}
    for name, v in flags.items():
        assert getattr(_ffi, name) == int(v), name
    assert (R.NO_CLEAN, R.ACROSS_COMPONENTS, R.COUNT_ONLY, R.NORMALS) == (1, 2, 4, 8)
    for name in ("cx_level1_simplify", "cx_level1_simplify_map", "cx_level1_simplify_map_download"):
        assert name in _ffi.SYMBOLS, name
        assert re.search(r"\bint %s\(cx_ctx\*" % name, text), name
    assert re.search(r"int cx_level1_simplify\(cx_ctx\* ctx, const double\* cell3, uint32_t flags, int64_t\* out_counts8, double\* q_out\);", sec)
    for want in ("[0] vertices", "[1] triangles", "[4] components", "[5] clamped coordinates", "[6] clusters", "[7] triangles with"):
        assert want in re.sub(r"\s*\n \*\s*", " ", sec), want
    assert _ffi.SIMPLIFY_KEYS == ("n_vertices", "n_triangles", "n_components", "n_clusters", "cell", "clamped")
    for cls in (tetrahedral.GridContour3d, tetrahedral.Delta3DContour, tetrahedral.LevelResult):
        assert callable(getattr(cls, "simplify")) and callable(getattr(cls, "simplify_map")) and callable(getattr(cls, "keep_components"))
    import inspect
    sig = inspect.signature(tetrahedral.GridContour3d.simplify)
    assert list(sig.parameters)[1:] == ["cell", "target_triangles", "by_component", "clean", "normals"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, None, True, True, "auto"]
