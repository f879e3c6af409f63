"""Host side of the clip (cx_clip.hip): the numpy restatement tests/clip_ref.py of the header's section "clipping" on hand-made meshes
with known answers and on two marched surfaces whose counts were worked out beforehand, the agreement of the Python constants and
declarations with the header text, and the argument checks of clip().  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

import clip_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "contourist_hip.h")


def _tetrahedron():
    "apex 0 above the base 1, 2, 3; wound outward"
    P = np.array([[0.0, 0.0, 3.0], [2.0, 0.0, 0.0], [-1.0, 1.7, 0.0], [-1.0, -1.7, 0.0]])
    T = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], dtype=np.int32)
    return P, T


def test_tetrahedron_cut_through_three_edges():
    P, T = _tetrahedron()
    s = P[:, 2]
    big = R.clip(P, T, s, 1.0, keep_below=True)           # the base's side
    cap = R.clip(P, T, s, 1.0)
    assert big["n_cut_vertices"] == cap["n_cut_vertices"] == 3 and big["n_cut_triangles"] == 3
    assert len(big["triangles"]) == 1 + 3 * 2 and len(cap["triangles"]) == 3
    assert len(big["points"]) == 3 + 3 and len(cap["points"]) == 1 + 3
    # the cut vertices lie on the plane, a third of the way down from the apex; keys: old index, then V + r
    assert np.allclose(big["points"][big["keys"] >= 4][:, 2], 1.0) and big["keys"].tolist() == [1, 2, 3, 4, 5, 6]
    assert cap["keys"].tolist() == [0, 4, 5, 6]
    # cut vertices in the order of the smallest corner number on their edge: edge {0,1} is corner 0, {0,2} corner 2 of triangle 0, {0,3} of triangle 1
    assert cap["cut_lo_hi"].tolist() == [[0, 1], [0, 2], [0, 3]]
    assert np.allclose(cap["cut_t"], 2.0 / 3.0)           # t runs from lo (the apex, d = 2) to hi (d = -1)
    assert np.allclose(big["cut_t"], 2.0 / 3.0)
    assert np.array_equal(big["map_lo_hi"][:3], [[1, 1], [2, 2], [3, 3]]) and np.all(big["map_t"][:3] == 0.0)
    # windings follow the source: all normals still point outward (the centroid is inside)
    for S in (big, cap):
        p, t = S["points"], S["triangles"]
        nrm = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
        assert np.all(np.sum(nrm * (p[t].mean(axis=1) - P.mean(axis=0)), axis=1) > 0)
    assert abs(R.area(big["points"], big["triangles"]) + R.area(cap["points"], cap["triangles"]) - R.area(P, T)) < 1e-14
    assert big["source"].tolist() == [0, 0, 1, 1, 2, 2, 3] and cap["source"].tolist() == [0, 1, 2]


def test_two_triangles_on_one_edge_share_one_cut_vertex():
    P = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, -1.0, 0.0]])
    T = np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32)
    S = R.clip(P, T, P[:, 0], 0.5)                          # x >= 0.5: the shared edge {0, 1} is cut once
    assert S["n_cut_vertices"] == 3 and S["n_cut_triangles"] == 2
    shared = [i for i, e in enumerate(S["cut_lo_hi"].tolist()) if e == [0, 1]]
    assert len(shared) == 1
    k = 4 + shared[0]
    assert np.count_nonzero(np.any(S["raw_triangles"] == k, axis=1)) == 3      # two triangles of one side, one of the other
    assert S["points"][S["keys"] == k].tolist() == [[0.5, 0.0, 0.0]]


def test_a_vertex_exactly_on_the_plane_makes_no_new_vertex():
    P = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [1.0, 1.0, 0.0], [1.0, -1.0, 0.0]])
    T = np.array([[0, 1, 2], [1, 0, 3]], dtype=np.int32)
    up = R.clip(P, T, P[:, 0], 1.0)                         # vertices 2 and 3 have d == 0
    assert up["n_on_cut"] == 2 and up["n_cut_vertices"] == 1        # only the edge {0, 1} is cut
    assert len(up["triangles"]) == 2 and up["keys"].tolist() == [1, 2, 3, 4]
    dn = R.clip(P, T, P[:, 0], 1.0, keep_below=True)
    assert dn["n_on_cut"] == 2 and dn["n_cut_vertices"] == 1 and len(dn["triangles"]) == 2
    # a triangle that only touches the plane from outside is dropped; from inside it is kept whole
    P2 = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    T2 = np.array([[0, 1, 2]], dtype=np.int32)
    assert len(R.clip(P2, T2, P2[:, 0], 1.0)["triangles"]) == 0
    assert len(R.clip(P2, T2, P2[:, 0], 1.0, keep_below=True)["triangles"]) == 1
    # an edge IN the plane with the third vertex outside: two inside, both on the cut: nothing is left
    P3 = np.array([[1.0, 1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 0.0, 0.0]])
    assert len(R.clip(P3, T2, P3[:, 0], 1.0)["triangles"]) == 0 and R.clip(P3, T2, P3[:, 0], 1.0)["n_cut_vertices"] == 0


def test_a_nan_scalar_drops_its_triangles_and_is_counted():
    P, T = _tetrahedron()
    s = P[:, 2].copy()
    s[1] = np.nan
    S = R.clip(P, T, s, -1.0)                               # everything else is inside
    assert S["n_nonfinite"] == 3 and S["triangles"].tolist() == [[0, 1, 2]] and S["keys"].tolist() == [0, 2, 3]
    s[1] = np.inf
    assert R.clip(P, T, s, -1.0)["n_nonfinite"] == 3
    assert R.clip(P, T, s, -1.0, keep_below=True)["n_nonfinite"] == 3


def test_keep_below_is_the_complement():
    rng = np.random.default_rng(5)
    import simplify_ref
    P, T = simplify_ref.sphere_mesh()
    s = rng.normal(size=len(P))
    up, dn = R.clip(P, T, s, 0.1), R.clip(P, T, s, 0.1, keep_below=True)
    assert up["n_cut_vertices"] == dn["n_cut_vertices"] and up["n_cut_triangles"] == dn["n_cut_triangles"]
    assert np.array_equal(up["cut_lo_hi"], dn["cut_lo_hi"]) and np.allclose(up["cut_t"], dn["cut_t"], rtol=0, atol=1e-15)
    # every cut triangle gives one triangle to one side and two to the other; every other triangle goes to exactly one side
    assert len(up["triangles"]) + len(dn["triangles"]) == len(T) + 2 * up["n_cut_triangles"]
    a = R.area(up["points"], up["triangles"]) + R.area(dn["points"], dn["triangles"])
    assert abs(a - R.area(P, T)) <= 1e-13 * R.area(P, T)


def test_carried_values_and_normals():
    import simplify_ref
    P, T = simplify_ref.sphere_mesh()
    N = (P - np.array((12.3, 11.6, 12.9))) / 9.7
    S = R.clip(P, T, P[:, 2], 13.0, normals=N)
    # the positions are themselves a carried attribute (up to the rounding of the other form of the interpolation)
    assert np.abs(R.carry(P, S["map_lo_hi"], S["map_t"]) - S["points"]).max() < 1e-13
    direct = (1.0 - S["map_t"]) * P[S["map_lo_hi"][:, 0], 2] + S["map_t"] * P[S["map_lo_hi"][:, 1], 2]
    assert np.array_equal(R.carry(P[:, 2], S["map_lo_hi"], S["map_t"]), direct)
    assert np.abs(np.linalg.norm(S["normals"], axis=1) - 1.0).max() < 1e-15
    assert np.array_equal(S["normals"][S["keys"] < len(P)], N[S["keys"][S["keys"] < len(P)]])

    class FakeContext(object):
        def level1_clip_map(self, device=False):
            return S["map_lo_hi"], S["map_t"]
    from contourist_amd import tetrahedral
    assert np.array_equal(tetrahedral._clip_values(P[:, 2], FakeContext()), direct)
    assert np.array_equal(tetrahedral._clip_values(P, FakeContext()), R.carry(P, S["map_lo_hi"], S["map_t"]))


def _marched(name):
    from oracle import level0, postpass
    if name == "sphere":
        I, J, K = np.meshgrid(*[np.arange(48, dtype=np.float64)] * 3, indexing="ij")
        A = (np.sqrt((I - 23.3) ** 2 + (J - 22.6) ** 2 + (K - 24.2) ** 2) - 15.4).astype(np.float32)
    else:
        I, J, K = np.meshgrid(np.arange(48.0), np.arange(48.0), np.arange(32.0), indexing="ij")
        A = (np.sqrt((np.sqrt((I - 23.4) ** 2 + (J - 23.7) ** 2) - 13.2) ** 2 + (K - 15.3) ** 2) - 5.1).astype(np.float32)
    O = level0.march3d(A, 0.0, diag_mode=1)
    L1 = postpass.level1_from_level0(level0.edge_keys_from_pairs(O["pairs"], A.shape), O["xyz"], O["tris"], np.array(A.shape) - 1)
    return np.asarray(L1["grid_points"]), np.asarray(L1["triangles"])


OBLIQUE = ((0.36, 0.48, 0.8), 0.36 * 23.3 + 0.48 * 22.6 + 0.8 * 24.2 + 1.37)


def test_counts_on_the_marched_sphere_and_torus():
    "the figures the restatement was vetted with: both sides of every cut, Euler numbers, shared cut curve, areas"
    P, T = _marched("sphere")
    a0 = R.area(P, T)
    s = R.plane_scalars(P, OBLIQUE[0])
    up, dn = R.clip(P, T, s, OBLIQUE[1]), R.clip(P, T, s, OBLIQUE[1], keep_below=True)
    assert (len(up["triangles"]), len(dn["triangles"]), up["n_cut_vertices"]) == (12851, 14763, 525)
    assert R.euler_and_boundary(up["triangles"]) == (1, 525) and R.euler_and_boundary(dn["triangles"]) == (1, 525)
    assert abs(R.area(up["points"], up["triangles"]) + R.area(dn["points"], dn["triangles"]) - a0) <= 1e-14 * a0
    s = R.plane_scalars(P, (1, 0, 0))
    up, dn = R.clip(P, T, s, 24.0), R.clip(P, T, s, 24.0, keep_below=True)
    assert up["n_on_cut"] == dn["n_on_cut"] == 208 and up["n_cut_vertices"] == dn["n_cut_vertices"] == 3
    assert R.euler_and_boundary(up["triangles"])[0] == 1 and R.euler_and_boundary(dn["triangles"])[0] == 1
    assert abs(R.area(up["points"], up["triangles"]) + R.area(dn["points"], dn["triangles"]) - a0) <= 1e-14 * a0
    P, T = _marched("torus")
    s = R.plane_scalars(P, OBLIQUE[0])
    assert R.euler_and_boundary(R.clip(P, T, s, OBLIQUE[1])["triangles"])[0] == 1                    # a cap
    assert R.euler_and_boundary(R.clip(P, T, s, OBLIQUE[1], keep_below=True)["triangles"])[0] == -1   # the torus minus a disc
    for n, off in (((1, 0, 0), 23.5), ((0, 0, 1), 15.3)):
        s = R.plane_scalars(P, n)
        assert R.euler_and_boundary(R.clip(P, T, s, off)["triangles"])[0] == 0
        assert R.euler_and_boundary(R.clip(P, T, s, off, keep_below=True)["triangles"])[0] == 0


def test_constants_and_declarations_agree_with_the_header():
    from contourist_amd import _ffi, tetrahedral
    text = open(HEADER).read()
    sec = text[text.index("---- clipping"):]
    sec = sec[:sec.index("cx_level1_clip_info(") + 100]
    flags = dict(re.findall(r"#define (CX_CLIP_\w+)\s+(\d+)u", sec))
    assert flags == {"CX_CLIP_NO_CLEAN": "1", "CX_CLIP_KEEP_BELOW": "2", "CX_CLIP_NORMALS": "4"}
    for name, v in flags.items():
        assert getattr(_ffi, name) == int(v), name
    assert (R.NO_CLEAN, R.KEEP_BELOW, R.NORMALS) == (1, 2, 4)
    for name in ("cx_level1_clip_plane", "cx_level1_clip_scalars", "cx_level1_clip_map", "cx_level1_clip_map_download", "cx_level1_clip_info"):
        assert name in _ffi.SYMBOLS, name
        assert re.search(r"\bint %s\(cx_ctx\*" % name, text), name
    assert "int cx_level1_clip_plane(cx_ctx* ctx, const double* plane4, uint32_t flags, int64_t* out_counts8);" in sec
    assert "int cx_level1_clip_scalars(cx_ctx* ctx, const double* scalars, int on_device, double threshold, uint32_t flags, int64_t* out_counts8);" in sec
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for want in ("[0] vertices", "[1] triangles", "[2] cut vertices", "[3] source triangles that were cut", "[4] components", "[5] n_nonfinite",
                 "[6] vertices with d == 0", "[7] triangles handed to the tail", "(V', 2) int32 and (V',) float64", "t = d[lo] / (d[lo] - d[hi])"):
        assert want in flat, want
    # the map's record layout as the binding reads it: pairs of int32, then float64
    lo_hi, t = np.zeros((5, 2), dtype=np.int32), np.zeros(5, dtype=np.float64)
    assert lo_hi.strides == (8, 4) and t.strides == (8,)
    assert _ffi.CLIP_KEYS == ("n_vertices", "n_triangles", "n_components", "n_cut_vertices", "n_cut_triangles", "n_nonfinite", "n_on_cut")
    for cls in (tetrahedral.GridContour3d, tetrahedral.Delta3DContour, tetrahedral.LevelResult):
        for m in ("clip", "clip_map", "clip_values"):
            assert callable(getattr(cls, m)), (cls, m)
        sig = inspect.signature(cls.clip)
        assert list(sig.parameters)[1:] == ["plane", "box", "field", "scalars", "value", "keep", "clean", "normals", "mins", "delta"]
        assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [None, None, None, None, 0.0, "above", True, "auto", None, None]


def test_argument_validation():
    from contourist_amd import tetrahedral
    A = tetrahedral._clip_args
    with pytest.raises(ValueError):
        A(None, None, None, None, "above")                               # no source
    with pytest.raises(ValueError):
        A(((1, 0, 0), 2.0), None, None, np.zeros(3), "above")           # two sources
    with pytest.raises(ValueError):
        A(((0, 0, 0), 2.0), None, None, None, "above")                   # zero normal
    with pytest.raises(ValueError):
        A(((1, np.nan, 0), 2.0), None, None, None, "above")
    with pytest.raises(ValueError):
        A(((1, 0, 0), 2.0), None, None, None, "sideways")
    with pytest.raises(ValueError):
        A(None, ((0, 0, 0), (1, 1, 1)), None, None, "below")
    kind, planes = A(((1.0, 2.0, 0.0), 3.0), None, None, None, "above")
    assert kind == "planes" and planes[0][0].tolist() == [1.0, 2.0, 0.0] and planes[0][1] == 3.0
    # world coordinates: n.(g * delta + mins) >= offset  <=>  (n * delta).g >= offset - n.mins
    kind, planes = A(((1.0, 2.0, 0.0), 3.0), None, None, None, "above", mins=(0.5, -1.0, 7.0), delta=(0.25, 0.5, 2.0))
    assert planes[0][0].tolist() == [0.25, 1.0, 0.0] and planes[0][1] == 3.0 - (0.5 - 2.0)
    kind, planes = A(None, ((1, 2, 3), (4, 5, 6)), None, None, "above")
    assert [(p[0].tolist(), p[1]) for p in planes] == [([1.0, 0.0, 0.0], 1.0), ([-1.0, -0.0, -0.0], -4.0), ([0.0, 1.0, 0.0], 2.0), ([-0.0, -1.0, -0.0], -5.0),
                                                       ([0.0, 0.0, 1.0], 3.0), ([-0.0, -0.0, -1.0], -6.0)]
    assert A(None, None, "B", None, "below") == ("field", "B")
    s = np.zeros(4)
    assert A(None, None, None, s, "above")[0] == "scalars"
