"""Host side of the vertex attributes: the mesh writers with normals and the ctypes declarations (no GPU)."""
import ctypes
import json
import struct

import numpy as np


def _mesh(seed=4, nv=37, nt=51):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((nv, 3))
    T = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)
    N = rng.standard_normal((nv, 3))
    N /= np.linalg.norm(N, axis=1)[:, None]
    return P, T, N


def _reference_ply(P, T, comment="contourist_amd isosurface"):
    "the bytes of the writer without normals, restated"
    header = ("ply\nformat binary_little_endian 1.0\ncomment %s\nelement vertex %d\n"
              "property double x\nproperty double y\nproperty double z\n"
              "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (comment, len(P), len(T)))
    body = P.astype("<f8").tobytes() + b"".join(struct.pack("<B3i", 3, *[int(x) for x in t]) for t in T)
    return header.encode("ascii") + body


def test_ply_round_trip_with_normals(tmp_path):
    from contourist_amd import mesh_io
    P, T, N = _mesh()
    path = str(tmp_path / "n.ply")
    mesh_io.write_ply(path, P, T, normals=N)
    P2, T2, N2 = mesh_io.read_ply(path, normals=True)
    assert np.array_equal(P2, P) and np.array_equal(T2, T) and np.array_equal(N2, N)
    P3, T3 = mesh_io.read_ply(path)                       # the optional three properties are skipped by a reader that does not ask
    assert np.array_equal(P3, P) and np.array_equal(T3, T)
    blob = open(path, "rb").read()
    head = blob[:blob.index(b"end_header\n")].decode("ascii")
    assert "property double z\nproperty double nx\nproperty double ny\nproperty double nz\nelement face" in head
    assert len(blob) == blob.index(b"end_header\n") + len(b"end_header\n") + len(P) * 48 + len(T) * 13


def test_default_arguments_keep_the_bytes(tmp_path):
    from contourist_amd import mesh_io
    P, T, _N = _mesh(seed=9)
    path = str(tmp_path / "plain.ply")
    mesh_io.write_ply(path, P, T)
    assert open(path, "rb").read() == _reference_ply(P, T)
    P2, T2, N2 = mesh_io.read_ply(path, normals=True)
    assert N2 is None and np.array_equal(P2, P) and np.array_equal(T2, T)
    g = str(tmp_path / "plain.gltf")
    mesh_io.write_gltf_bin(g, P, T)
    assert open(str(tmp_path / "plain.bin"), "rb").read() == P.astype("<f4").tobytes() + T.astype("<u4").tobytes()
    doc = json.load(open(g))
    assert doc["meshes"][0]["primitives"][0]["attributes"] == {"POSITION": 0} and len(doc["bufferViews"]) == 2 and len(doc["accessors"]) == 2


def test_gltf_round_trip_with_normals(tmp_path):
    from contourist_amd import mesh_io
    P, T, N = _mesh(seed=6)
    g = str(tmp_path / "n.gltf")
    mesh_io.write_gltf_bin(g, P, T, normals=N)
    doc = json.load(open(g))
    blob = open(str(tmp_path / "n.bin"), "rb").read()
    assert doc["buffers"][0]["byteLength"] == len(blob) == len(P) * 24 + T.size * 4
    prim = doc["meshes"][0]["primitives"][0]
    assert prim["attributes"] == {"POSITION": 0, "NORMAL": 2} and prim["indices"] == 1 and len(doc["bufferViews"]) == 3

    def section(accessor, dtype):
        a = doc["accessors"][accessor]
        v = doc["bufferViews"][a["bufferView"]]
        return a, np.frombuffer(blob[v["byteOffset"]:v["byteOffset"] + v["byteLength"]], dtype=dtype)
    a, pos = section(0, "<f4")
    assert np.array_equal(pos.reshape(-1, 3), P.astype(np.float32))
    a, nrm = section(2, "<f4")
    assert a == {"bufferView": 2, "componentType": 5126, "count": len(P), "type": "VEC3"}
    assert np.array_equal(nrm.reshape(-1, 3), N.astype(np.float32))
    a, idx = section(1, "<u4")
    assert a["count"] == T.size and np.array_equal(idx.reshape(-1, 3), T.astype(np.uint32))


def test_ffi_declares_the_new_symbols():
    from contourist_amd import _ffi
    new = ["cx_level0_normals", "cx_level0_normals_download", "cx_level1_normals", "cx_level1_normals_download",
           "cx_level0_sample_grid", "cx_level1_sample_grid"]
    for name in new:
        assert name in _ffi.SYMBOLS
    L = _ffi.load()
    vp = ctypes.c_void_p
    want = {
        "cx_level0_normals": [vp, vp, ctypes.POINTER(vp)],
        "cx_level0_normals_download": [vp, vp, vp],
        "cx_level1_normals": [vp, vp, ctypes.POINTER(vp)],
        "cx_level1_normals_download": [vp, vp, vp],
        "cx_level0_sample_grid": [vp, vp, ctypes.c_int32, ctypes.c_int, ctypes.POINTER(vp), vp],
        "cx_level1_sample_grid": [vp, vp, ctypes.c_int32, ctypes.c_int, ctypes.POINTER(vp), vp],
    }
    for name, args in want.items():
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args, name
    assert _ffi.CX_ERR_INVALID == -1 and _ffi.CX_ERR_UNSUPPORTED == -6
    for method in ("level0_normals", "level1_normals", "level0_sample", "level1_sample"):
        assert callable(getattr(_ffi.Context, method))
