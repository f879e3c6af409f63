"""Host side of the Level-1 topology (cx_topo.hip): the record layouts of the ctypes / numpy mirrors against the text of
include/contourist_hip.h, the numpy reference tests/topology_ref.py on hand-made meshes whose answers are known, and the genus /
boundary_loops selectors of keep_components on a made-up table.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import topology_meshes as meshes
import topology_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "contourist_hip.h")
CALLS = ["cx_level1_topology", "cx_level1_topology_download", "cx_level1_boundary_loops", "cx_level1_boundary_loops_download"]


def _header_layout(struct):
    "[(name, offset, size)] of a record as the header declares it (natural alignment), and its size"
    text = open(HEADER).read()
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S)
    assert m, struct + " is not declared in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    sizes = {"int64_t": 8, "int32_t": 4, "uint32_t": 4}
    fields, at = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for name in names.split(","):
            size = sizes[ctype]
            at = (at + size - 1) // size * size
            fields.append((name.strip(), at, size))
            at += size
    return fields, (at + 7) // 8 * 8


@pytest.mark.parametrize("struct,total,dtype_name", [("cx_topology", 64, "TOPOLOGY_DTYPE"), ("cx_loop", 16, "LOOP_DTYPE")])
def test_record_layouts_match_the_header(struct, total, dtype_name):
    from contourist_amd import _ffi
    fields, size = _header_layout(struct)
    cls, dtype = getattr(_ffi, struct), getattr(_ffi, dtype_name)
    assert size == total == ctypes.sizeof(cls) == dtype.itemsize
    assert [f[0] for f in fields] == [f[0] for f in cls._fields_] == list(dtype.names)
    for name, offset, nbytes in fields:
        c = getattr(cls, name)
        assert (c.offset, c.size) == (offset, nbytes), name
        dt, off = dtype.fields[name][:2]
        assert (off, dt.itemsize) == (offset, nbytes), name
    assert dtype == getattr(topology_ref, dtype_name)                 # the reference writes the same records


def test_declarations_present():
    from contourist_amd import _ffi
    text = open(HEADER).read()
    for name in CALLS:
        assert name in _ffi.SYMBOLS, name
        assert re.search(r"\bint %s\(cx_ctx\*" % name, text), name


def _ref(mesh):
    _P, T = mesh
    return topology_ref.topology(T, meshes.edge_components(T))


def _row(table, c=0):
    return {k: int(table[k][c]) for k in table.dtype.names}


def test_reference_closed_meshes():
    t, loops, verts = _ref(meshes.tetrahedron())
    assert len(t) == 1 and len(loops) == 0 and len(verts) == 0
    assert _row(t) == dict(triangles=4, vertices=4, edges=6, boundary_edges=0, nonmanifold_edges=0, euler=2, boundary_loops=0, genus=0,
                           nonsimple_loops=0, reserved=0)
    t, loops, verts = _ref(meshes.torus_grid(4))
    assert _row(t) == dict(triangles=32, vertices=16, edges=48, boundary_edges=0, nonmanifold_edges=0, euler=0, boundary_loops=0, genus=1,
                           nonsimple_loops=0, reserved=0)
    assert len(loops) == 0


def test_reference_annulus():
    P, T = meshes.annulus()
    t, loops, verts = _ref((P, T))
    r = _row(t)
    assert (r["triangles"], r["vertices"], r["edges"], r["euler"], r["boundary_loops"], r["genus"], r["nonsimple_loops"]) == (12, 12, 24, 0, 2, 0, 0)
    assert r["boundary_edges"] == 12 and len(verts) == 12
    assert loops["simple"].tolist() == [1, 1] and loops["count"].tolist() == [6, 6] and loops["first"].tolist() == [0, 6]
    # the smallest 3t+k of a boundary edge is edge 0 of triangle 0, (outer 1' -> outer 2'): that loop comes first, in that direction
    assert verts[:6].tolist() == [6, 7, 8, 9, 10, 11]
    # the inner ring's first boundary edge is k = 1 of triangle 1 = (7, 1, 0): it runs 1 -> 0
    assert verts[6:].tolist() == [1, 0, 5, 4, 3, 2]


def test_reference_moebius_book_wheel():
    t, loops, verts = _ref(meshes.moebius())
    r = _row(t)
    assert (r["vertices"], r["edges"], r["triangles"], r["euler"], r["boundary_edges"], r["boundary_loops"], r["genus"]) == (5, 10, 5, 0, 5, 1, -1)
    assert loops["simple"].tolist() == [1] and verts.tolist() == [2, 0, 3, 1, 4]      # from edge k = 2 of triangle 0: 2 -> 0
    t, loops, verts = _ref(meshes.book())
    r = _row(t)
    assert (r["nonmanifold_edges"], r["genus"], r["edges"], r["boundary_edges"], r["boundary_loops"], r["nonsimple_loops"]) == (1, -1, 7, 6, 1, 1)
    assert loops["simple"].tolist() == [0] and verts.tolist() == [1, 2, 0, 3, 1, 4]   # tails in ascending 3t+k
    t, loops, verts = _ref(meshes.pinched_wheel())
    r = _row(t)
    assert (r["vertices"], r["edges"], r["triangles"], r["euler"]) == (13, 30, 16, -1)
    assert (r["boundary_loops"], r["nonsimple_loops"], r["nonmanifold_edges"], r["boundary_edges"]) == (2, 1, 0, 12)
    assert r["genus"] == -1                                                           # 2 - (-1) - 2 = 1 is odd
    assert loops["simple"].tolist() == [1, 0] and loops["count"].tolist() == [6, 6]
    assert verts[:6].tolist() == [6, 7, 8, 9, 10, 11]
    inner = {frozenset(e) for e in [(12, 2), (2, 3), (3, 12), (12, 5), (5, 0), (0, 12)]}          # a-3, 3-4, 4-a, a-6, 6-1, 1-a
    P, T = meshes.pinched_wheel()
    uses = {}
    for tt, row in enumerate(T):
        for k in range(3):
            uses.setdefault(frozenset((int(row[k]), int(row[(k + 1) % 3]))), []).append((3 * tt + k, int(row[k])))
    want = sorted(u[0] for e, u in uses.items() if e in inner)
    assert all(len(uses[e]) == 1 for e in inner)
    assert verts[6:].tolist() == [tail for _e, tail in want]


def test_reference_shared_vertex_counts_in_both():
    P, T = meshes.two_touching_triangles()
    lab = meshes.edge_components(T)
    assert lab.tolist() == [0, 1]
    t, loops, verts = topology_ref.topology(T, lab)
    assert t["vertices"].tolist() == [3, 3] and t["vertices"].sum() == len(P) + 1
    assert t["euler"].tolist() == [1, 1] and t["boundary_loops"].tolist() == [1, 1] and t["genus"].tolist() == [0, 0]
    assert loops["component"].tolist() == [0, 1] and verts.tolist() == [0, 1, 2, 0, 3, 4]
    e = topology_ref.topology(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32))
    assert [len(x) for x in e] == [0, 0, 0]


def test_topology_selectors():
    from contourist_amd import _ffi
    from contourist_amd.surface_geometry import select_components as sel
    T = np.zeros(5, dtype=_ffi.COMPONENT_DTYPE)
    T["triangles"] = [10, 500, 30, 500, 4]
    T["closed"] = [1, 1, 0, 0, 1]
    topo = np.zeros(5, dtype=_ffi.TOPOLOGY_DTYPE)
    topo["genus"] = [0, 1, 0, -1, 3]
    topo["boundary_loops"] = [0, 0, 2, 1, 0]
    assert sel(T, topology=topo).tolist() == [True] * 5
    assert sel(T, topology=topo, genus=1).tolist() == [False, True, False, False, False]
    assert sel(T, topology=topo, genus=(0, 1)).tolist() == [True, True, True, False, False]
    assert sel(T, topology=topo, genus=(1, 3)).tolist() == [False, True, False, False, True]
    assert sel(T, topology=topo, boundary_loops=0).tolist() == [True, True, False, False, True]
    assert sel(T, topology=topo, boundary_loops=(1, 2)).tolist() == [False, False, True, True, False]
    assert sel(T, topology=topo, genus=0, boundary_loops=0, min_triangles=5).tolist() == [True, False, False, False, False]
    assert sel(T, largest=1, topology=topo, genus=(0, 9)).tolist() == [False, True, False, False, False]
    assert sel(T, largest=1, closed=True).tolist() == [False, True, False, False, False]            # the old selectors as before
    with pytest.raises(ValueError):
        sel(T, genus=1)
    with pytest.raises(ValueError):
        sel(T, topology=topo[:3], boundary_loops=0)
