"""Host side of the rim caps (cx_cap.hip): the numpy restatement tests/cap_ref.py of the header's section "rim caps" on fields with known
answers -- Level 0 from oracle.level0.march3d, the cap from cap_ref, Level 1 from oracle.postpass.level1_from_level0 --, the agreement
of the Python constants and declarations with the header text, and the argument checks of cap_rim().  No GPU.

The fields of the closedness assertions have no sample within 1e-3 of the isovalue and no crossing the march skipped; both are asserted.
The sphere of the issue (radius 9 about (3, 10, 10) in 21^3) has lattice points at distance exactly 9, so it cannot meet the first
condition: the closedness assertions use the same sphere with its centre moved off the lattice (cap_ref.SPHERE_OFF); the sphere as
written is the parity-only case of tests/test_gpu_cap.py."""
import inspect
import os
import re

import numpy as np
import pytest

import cap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "contourist_hip.h")

_level0 = {}


def _marched(name):
    "the oracle's Level-0 mesh of a field, once: (samples, value, keys, float64 points, triangles wound low -> high)"
    if name not in _level0:
        from oracle import level0
        A, v = R.field(name)
        O = level0.march3d(A, v, diag_mode=1)
        keys = level0.edge_keys_from_pairs(O["pairs"], A.shape)
        _level0[name] = (A, v, keys, O["xyz"], R.wind_low_to_high(A, v, O["pairs"], O["xyz"], O["tris"]))
    return _level0[name]


def _capped(name, faces, side):
    A, v, keys0, xyz0, tris0 = _marched(name)
    return R.capped_level0(A, v, R.faces_mask(faces), side, keys0, xyz0, tris0)


def _level1(name, faces, side):
    from oracle import postpass
    A = R.field(name)[0]
    keys, xyz, tris, C = _capped(name, faces, side)
    L1 = postpass.level1_from_level0(keys, xyz, tris, np.array(A.shape) - 1)
    return np.asarray(L1["grid_points"]), np.asarray(L1["triangles"]), C


def _closedness_conditions(name, C):
    A, v = R.field(name)
    assert np.abs(A.astype(np.float64) - v).min() > 1e-3, name
    assert C["counts"][2] == 0, (name, C["counts"])


def test_no_crossing_at_all():
    keys, xyz, tris, C = _capped("constant", "all", "below")
    _closedness_conditions("constant", C)
    a, b, c = 4, 3, 2
    assert C["counts"].tolist() == [5 * 4 * 3 - 3 * 2 * 1, 4 * (a * b + b * c + c * a), 0, 0] == [54, 104, 0, 0]
    assert len(C["keys"]) == 54 and np.all(C["keys"] & 7 == 0) and np.all(np.diff(C["keys"].astype(np.int64)) > 0)
    boundary, nonmanifold, incoherent, euler = R.edge_uses(tris)
    assert (boundary, nonmanifold, incoherent, euler) == (0, 0, 0, 2)
    assert R.signed_volume(xyz, tris) == 4.0 * 3.0 * 2.0          # "below": the normals point out of the solid
    P, T, _C = _level1("constant", "all", "below")
    assert len(P) == 54 and len(T) == 104 and R.edge_uses(T) == (0, 0, 0, 2)
    keys, xyz, tris, C = _capped("constant", "all", "above")
    assert C["counts"].tolist() == [0, 0, 0, 0] and len(C["keys"]) == 0 and len(tris) == 0


@pytest.mark.parametrize("side,volume", [("above", 4.5 * 5 * 4), ("below", 2.5 * 5 * 4)])
def test_plane_field(side, volume):
    keys, xyz, tris, C = _capped("plane", "all", side)
    _closedness_conditions("plane", C)
    assert R.edge_uses(tris) == (0, 0, 0, 2)
    # the march's normals point from f < v to f >= v: into the solid of "above" (negative signed volume), out of the solid of "below"
    assert R.signed_volume(xyz, tris) == (-volume if side == "above" else volume)
    P, T, _C = _level1("plane", "all", side)
    assert R.edge_uses(T) == (0, 0, 0, 2)
    assert abs(R.signed_volume(P, T)) == volume
    # the rim edges between the planes i = 2 and i = 3: on each j-face 5 straight and 4 diagonal ones, on each k-face 6 and 5, less the
    # four along the box edges that two faces share
    assert C["counts"][3] == 2 * (5 + 4) + 2 * (6 + 5) - 4 == 36


def test_sphere_cut_by_the_rim():
    A, v, keys0, xyz0, tris0 = _marched("sphere")
    assert R.edge_uses(tris0)[0] > 0                               # uncapped: open
    for side in ("above", "below"):
        keys, xyz, tris, C = _capped("sphere", "all", side)
        _closedness_conditions("sphere", C)
        assert R.edge_uses(tris) == (0, 0, 0, 2), side
        P, T, _C = _level1("sphere", "all", side)
        assert R.edge_uses(T) == (0, 0, 0, 2), side
    # the ball reaches only the face i = 0 ("-x"): its volume is that of the sphere less the segment beyond the face, to the
    # accuracy of a piecewise-linear surface of this resolution
    h = 9.0 - R.SPHERE_OFF[0]
    exact = 4.0 / 3.0 * np.pi * 9.0 ** 3 - np.pi * h * h * (3 * 9.0 - h) / 3.0
    keys, xyz, tris, C = _capped("sphere", "all", "above")
    assert abs(-R.signed_volume(xyz, tris) / exact - 1.0) < 0.02


def test_omitted_face_keeps_its_loops():
    "two balls, one cut by -x, one by +y: with -x omitted the loops that remain lie in the face i = 0"
    I, J, K = R._ijk((21, 21, 21))
    ball = lambda c, r: r - np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2)
    A = np.maximum(ball((2.33, 6.16, 9.83), 5.0), ball((14.20, 18.41, 10.11), 5.0)).astype(np.float32)
    from oracle import level0
    O = level0.march3d(A, 0.0, diag_mode=1)
    keys0 = level0.edge_keys_from_pairs(O["pairs"], A.shape)
    tris0 = R.wind_low_to_high(A, 0.0, O["pairs"], O["xyz"], O["tris"])
    assert np.abs(A).min() > 1e-3
    keys, xyz, tris, C = R.capped_level0(A, 0.0, R.faces_mask("all"), "above", keys0, O["xyz"], tris0)
    assert C["counts"][2] == 0 and R.edge_uses(tris) == (0, 0, 0, 4)        # two closed pieces
    keys, xyz, tris, C = R.capped_level0(A, 0.0, R.faces_mask(["+x", "-y", "+y", "-z", "+z"]), "above", keys0, O["xyz"], tris0)
    t = np.asarray(tris)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    und, cnt = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1), axis=0, return_counts=True)
    open_edges = und[cnt == 1]
    assert len(open_edges) > 0 and np.all(xyz[open_edges.ravel()][:, 0] == 0.0)


def test_each_vertex_once():
    for name, side in (("constant", "below"), ("plane", "above"), ("sphere", "below"), ("noise_14x20x26", "above")):
        A, v = R.field(name)
        keys, xyz, tris, C = _capped(name, "all", side)
        assert len(np.unique(keys)) == len(keys), name
        ck = C["keys"].astype(np.int64)
        assert np.all(np.diff(ck) > 0), name
        # the eight corners of the box lie on three faces, the points of its twelve edges on two: one vertex each
        ins = R.inside_mask(A, v, side)
        n = A.shape
        lin = np.arange(A.size).reshape(n)
        rim = np.zeros(n, dtype=bool)
        rim[0], rim[-1], rim[:, 0], rim[:, -1], rim[:, :, 0], rim[:, :, -1] = True, True, True, True, True, True
        want = np.sort(lin[rim & ins]) * 8
        assert np.array_equal(ck[ck & 7 == 0], want), name            # every inside rim point is a corner of some face-triangle
        assert np.array_equal(R.points(A, v, ck[ck & 7 == 0]), np.stack(np.unravel_index(want // 8, n), axis=1).astype(np.float64))


@pytest.mark.parametrize("name", ["plane", "sphere", "noise_14x20x26", "noise_u8"])
def test_coherent_winding_of_the_raw_concatenation(name):
    """before any orientation step, with the march's triangles wound low -> high as the device winds them (cap_ref.wind_low_to_high needs
    triangles with an area: the sphere with samples equal to the isovalue, whose crossings coincide there, is left to the device test)"""
    for side in ("above", "below"):
        for mask in R.MASKS:
            keys, xyz, tris, C = _capped(name, mask, side)
            boundary, nonmanifold, incoherent, _euler = R.edge_uses(tris)
            if C["counts"][2] == 0:
                assert (nonmanifold, incoherent) == (0, 0), (name, side, mask)
                if mask == 0x3F:
                    assert boundary == 0, (name, side)
            assert C["counts"][1] == len(C["triangles"]) and C["counts"][0] + C["counts"][2] == len(C["keys"])


def test_constants_and_declarations_agree_with_the_header():
    from contourist_amd import _ffi, tetrahedral
    text = open(HEADER).read()
    sec = text[text.index("---- rim caps"):]
    sec = sec[:sec.index("int cx_postprocess3d_capped(") + 100]
    defs = dict(re.findall(r"#define (CX_CAP_\w+)\s+(\d+)u", sec))
    assert defs == {"CX_CAP_BELOW": "1", "CX_CAP_ALL_FACES": "63"}
    for name, v in defs.items():
        assert getattr(_ffi, name) == int(v), name
    assert (R.SIDE_BELOW, R.ALL_FACES) == (1, 63)
    for name in ("cx_cap3d", "cx_cap3d_download", "cx_cap3d_info", "cx_postprocess3d_capped"):
        assert name in _ffi.SYMBOLS, name
        assert re.search(r"\bint %s\(cx_ctx\*" % name, text), name
    assert "int cx_cap3d(cx_ctx* ctx, uint32_t faces, uint32_t flags, int64_t* counts4);" in sec
    assert "int cx_cap3d_download(cx_ctx* ctx, uint32_t* keys, int32_t* tris);" in sec
    assert "int cx_postprocess3d_capped(cx_ctx* ctx, uint32_t flags, int64_t* out_counts);" in sec
    flat = re.sub(r"\s*\n \*\s*", " ", sec)
    for want in ("bit 0: i = 0, bit 1: i = n0-1, bit 2: j = 0, bit 3: j = n1-1, bit 4: k = 0, bit 5: k = n2-1",
                 "[0] lattice-point vertices, [1] cap triangles, [2] crossings the march had not emitted, [3] rim edges with a crossing",
                 "(linear index << 3) | 0", "in ascending key", "(face number, square's linear index in the face, triangle 0 / 1, piece 0 / 1)",
                 "(p_i, c(i,j), c(i,k))", "(c(i,j), p_j, p_k) and (c(i,j), p_k, c(k,i))", "ABOVE: faces 1, 2, 5; BELOW: faces 0, 3, 4",
                 "direction 3 on an i-face, 5 on a j-face, 6 on a k-face"):
        assert want in flat, want
    assert _ffi.CAP_KEYS == R.COUNT_KEYS == ("n_lattice_vertices", "n_cap_triangles", "n_missing_crossings", "n_rim_crossings")
    assert _ffi.CAP_FACES == R.FACE_NAMES == ("-x", "+x", "-y", "+y", "-z", "+z")
    # the reversed faces as the header lists them
    assert [f for f in range(6) if R.reversed_face(f, "above")] == [1, 2, 5] and [f for f in range(6) if R.reversed_face(f, "below")] == [0, 3, 4]
    for cls in (tetrahedral.GridContour3d, tetrahedral.Delta3DContour, tetrahedral.TriangulatedIsosurfaces):
        sig = inspect.signature(cls.cap_rim)
        assert list(sig.parameters)[1:] == ["faces", "side"] and [p.default for p in list(sig.parameters.values())[1:]] == ["all", "above"]
    assert inspect.signature(tetrahedral.MultiLevelIsosurfaces.levels).parameters["cap"].default is None
    for m in ("cap3d", "download_cap", "postprocess3d_capped"):
        assert callable(getattr(_ffi.Context, m)), m
    lo, hi = tetrahedral.unpack_edge_ids(np.array([8 * 7 + 0, 8 * 7 + 5]), (3, 4, 5))
    assert lo.tolist() == [[0, 1, 2], [0, 1, 2]] and hi.tolist() == [[0, 1, 2], [1, 1, 3]]


def test_argument_validation():
    from contourist_amd import _ffi, tetrahedral
    assert _ffi.cap_faces_mask("all") == 63 and _ffi.cap_faces_mask(0x2A) == 0x2A and _ffi.cap_faces_mask(0) == 0
    assert _ffi.cap_faces_mask(["-x", "+z"]) == 0x21 and _ffi.cap_faces_mask("+y") == 8
    assert [_ffi.cap_faces_mask([n]) for n in _ffi.CAP_FACES] == [1, 2, 4, 8, 16, 32]
    for bad in (64, -1, ["x"], ["-x", "up"]):
        with pytest.raises(ValueError):
            _ffi.cap_faces_mask(bad)
    assert _ffi.cap_side_flags("above") == 0 and _ffi.cap_side_flags("below") == _ffi.CX_CAP_BELOW
    with pytest.raises(ValueError):
        _ffi.cap_side_flags("inside")
    A = np.zeros((5, 4, 3), dtype=np.float32)
    G = tetrahedral.GridContour3d
    # every refusal comes before the device is touched (no context is made here)
    with pytest.raises(ValueError):
        G((4, 3, 2), A, 1.0).cap_rim(["top"])
    with pytest.raises(ValueError):
        G((4, 3, 2), A, 1.0).cap_rim("all", side="outside")
    with pytest.raises(NotImplementedError, match="end points"):
        G((4, 3, 2), A, 1.0, segment_endpoints=[((0, 0, 0), (1, 1, 1))]).cap_rim()
    with pytest.raises(NotImplementedError, match="voxel_range"):
        G((4, 3, 2), A, 1.0, voxel_range=((1, 1, 1), (3, 2, 1))).cap_rim()
    with pytest.raises(NotImplementedError, match="linear_interpolate"):
        G((4, 3, 2), A, 1.0, linear_interpolate=False, function=lambda i, j, k: 0.0).cap_rim()
    m = G((4, 3, 2), A, 1.0)
    m.smooth = 0.5
    with pytest.raises(NotImplementedError, match="smooth"):
        m.cap_rim()
    m = G((4, 3, 2), A, 1.0)
    m.MAX_SAMPLES_PER_EXTRACTION = 16
    with pytest.raises(NotImplementedError, match="slabs"):
        m.cap_rim()
    m = G((4, 3, 2), A, 1.0)
    assert m.cap_rim(None) is None and m._cap is None
