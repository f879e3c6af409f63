"""Host side of the Level-1 components (cx_comp.hip): the record layout of the ctypes / numpy mirrors against the text of
include/contourist_hip.h, the permutation that carries triangle labels into the order of the sorted rows, and the selectors of
keep_components on a made-up table.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "contourist_hip.h")
CALLS = ["cx_level1_components", "cx_level1_components_download", "cx_level1_component_labels", "cx_level1_component_labels_download",
         "cx_level1_keep_components"]


def _header_layout():
    "[(name, offset, size)] of cx_component as the header declares it: natural alignment of int64_t / double / int32_t"
    text = open(HEADER).read()
    m = re.search(r"typedef struct cx_component \{(.*?)\} cx_component;", text, re.S)
    assert m, "cx_component is not declared in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    sizes = {"int64_t": 8, "double": 8, "int32_t": 4}
    fields, at = [], 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        for name in names.split(","):
            name = name.strip()
            count = 1
            a = re.match(r"(\w+)\[(\d+)\]$", name)
            if a:
                name, count = a.group(1), int(a.group(2))
            size = sizes[ctype]
            at = (at + size - 1) // size * size
            fields.append((name, at, size * count))
            at += size * count
    return fields, (at + 7) // 8 * 8


def test_record_layout_matches_the_header():
    from contourist_amd import _ffi
    fields, total = _header_layout()
    assert total == 128 == ctypes.sizeof(_ffi.cx_component) == _ffi.COMPONENT_DTYPE.itemsize
    assert [f[0] for f in fields] == [f[0] for f in _ffi.cx_component._fields_] == list(_ffi.COMPONENT_DTYPE.names)
    for name, offset, size in fields:
        c = getattr(_ffi.cx_component, name)
        assert (c.offset, c.size) == (offset, size), name
        dt, off = _ffi.COMPONENT_DTYPE.fields[name][:2]
        assert (off, dt.itemsize) == (offset, size), name


def test_declarations_present():
    from contourist_amd import _ffi
    text = open(HEADER).read()
    for name in CALLS:
        assert name in _ffi.SYMBOLS, name
        assert re.search(r"\bint %s\(cx_ctx\*" % name, text), name


def test_label_permutation_is_the_row_sort():
    from contourist_amd import surface_geometry
    rng = np.random.default_rng(5)
    tris = rng.integers(0, 40, size=(500, 3)).astype(np.int32)          # many equal leading indices: ties go to columns 1 and 2
    order = surface_geometry.row_order(tris)
    assert np.array_equal(tris[order], surface_geometry.sort_rows(tris))
    assert np.array_equal(surface_geometry.sort_rows(tris), np.array(sorted(map(tuple, tris.tolist())), dtype=np.int32))
    labels = rng.integers(0, 7, size=len(tris)).astype(np.int32)
    # a label travels with its row: look every sorted row up among the rows that carry the permuted label
    for row, lab in zip(tris[order][::37], labels[order][::37]):
        assert any(np.array_equal(row, r) for r in tris[labels == lab])
    assert len(surface_geometry.row_order(np.zeros((0, 3), dtype=np.int32))) == 0
    assert surface_geometry.sort_rows(np.zeros((0, 3), dtype=np.int32)).shape == (0, 3)


def _table():
    from contourist_amd import _ffi
    T = np.zeros(6, dtype=_ffi.COMPONENT_DTYPE)
    T["triangles"] = [10, 500, 30, 500, 4, 80]
    T["area"] = [1.0, 90.0, 2.5, 70.0, 0.1, 9.0]
    T["closed"] = [1, 1, 0, 0, 1, 1]
    return T


def test_selectors_combine_with_and():
    from contourist_amd.surface_geometry import select_components as sel
    T = _table()
    assert sel(T).tolist() == [True] * 6
    assert sel(T, largest=1).tolist() == [False, True, False, False, False, False]              # the tie 500 / 500 goes to the smaller id
    assert sel(T, largest=3).tolist() == [False, True, False, True, False, True]
    assert sel(T, largest=0).tolist() == [False] * 6 and sel(T, largest=99).tolist() == [True] * 6
    assert sel(T, min_triangles=30).tolist() == [False, True, True, True, False, True]
    assert sel(T, min_area=2.5).tolist() == [False, True, True, True, False, True]
    assert sel(T, closed=True).tolist() == [True, True, False, False, True, True]
    assert sel(T, closed=False).tolist() == [False, False, True, True, False, False]
    assert sel(T, mask=[1, 0, 1, 1, 1, 1], largest=3, closed=False).tolist() == [False, False, False, True, False, False]
    assert sel(T, largest=2, min_triangles=30, closed=True).tolist() == [False, True, False, False, False, False]
    with pytest.raises(ValueError):
        sel(T, mask=[True, False])
    assert sel(T[:0]).shape == (0,)
