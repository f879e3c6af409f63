"""What a context's Level-1 state holds after every producer, as every reader sees it (cx_post.h: the record, begin / publish).

One small 3-D field (13x11x12: two closed blobs and a sheet the rim cuts open) and one 4-D field (6x7x8x5).  For every producer a
fresh context runs it, then every reader is called once and the class of its return is noted (OK / INVALID / STATE / UNSUPPORTED).

RECORDED was printed by walk() on the commit BEFORE the state record existed, on the device, twice with the same output: per producer
the readers' classes, the counts the producer returned, a SHA-256 of every array of the mesh, and cx_device_bytes of the context after
the walk.  Every array was bit-stable between the two runs but the morph's segments and triangles, whose segment ids follow the slots
of a hash table: those two are hashed in a canonical form (_canonical_morph), which was stable.  The readers of one dimensionality
after a post-pass of the other were NOT run there (they read the other pass's buffers by the wrong counts): None in RECORDED,
CX_ERR_STATE by design (expected())."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE3, VALUE3 = (13, 11, 12), 0.0
SHAPE4, VALUE4 = (6, 7, 8, 5), 0.0
ROOM = 1 << 16           # rows of every host buffer a reader may write into (the meshes here have a few hundred vertices)

READERS = ("download", "keys", "device_ptrs", "write", "normals", "curvature", "sample", "components", "component_labels", "topology",
           "simplify_map", "clip_map", "download_4d")
PRODUCERS = ("postprocess3d", "postprocess3d_noclean", "capped", "mesh", "shard_begin", "shard_finish", "simplify", "simplify_dry",
             "simplify_normals", "clip_plane", "keep_subset", "keep_all", "surface_geometry", "level0_points", "extract3d", "postprocess4d",
             "morph_triangles")
PRODUCERS_4D = ("postprocess4d", "morph_triangles")


def field3():
    "two closed blobs (inside = low) and a sheet near the top of the last axis that the array's rim cuts open; no sample equals the isovalue"
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE3], indexing="ij")
    a = np.sqrt((i - 3.21) ** 2 + (j - 3.13) ** 2 + (k - 3.37) ** 2) - 2.13
    b = np.sqrt((i - 8.73) ** 2 + (j - 6.91) ** 2 + (k - 4.11) ** 2) - 2.31
    sheet = 9.29 + 0.07 * np.sin(0.9 * i + 0.4 * j) - k
    return np.minimum(np.minimum(a, b), sheet).astype(np.float32)


def field4():
    i, j, k, t = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in SHAPE4], indexing="ij")
    return (np.sqrt((i - 2.43) ** 2 + (j - 3.11) ** 2 + (k - 3.57) ** 2 + (t - 2.21) ** 2) - 1.73).astype(np.float32)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _cls(rc):
    from contourist_amd import _ffi
    return {_ffi.CX_OK: "OK", _ffi.CX_ERR_INVALID: "INVALID", _ffi.CX_ERR_STATE: "STATE", _ffi.CX_ERR_UNSUPPORTED: "UNSUPPORTED"}.get(rc, "rc%d" % rc)


_inputs = {}


def inputs():
    "what the producers that take a caller's mesh are fed, computed once on a context of its own and never changed"
    if not _inputs:
        from contourist_amd import _ffi
        ctx = _ffi.Context()
        ctx.upload_grid(field3())
        c = ctx.extract3d(VALUE3)
        keys0, _t, tris0 = ctx.download_level0_records(c)
        pts0 = ctx.level0_points_f64(c)
        order = np.argsort(keys0, kind="stable")          # cx_postprocess3d_mesh: vertices in ascending edge-id order
        inv = np.empty(len(order), dtype=np.int32)
        inv[order] = np.arange(len(order), dtype=np.int32)
        _inputs["mesh"] = (pts0[order].copy(), inv[np.asarray(tris0).reshape(-1, 3)].copy())
        p = ctx.postprocess3d(0)
        _inputs["level1"] = ctx.download_level1(p)
        ctx.close()
    return _inputs


def fresh3():
    from contourist_amd import _ffi
    ctx = _ffi.Context()
    ctx.upload_grid(field3())
    return ctx, ctx.extract3d(VALUE3)


def march4(ctx):
    ctx.upload_grid4d(field4())
    return ctx.extract4d(VALUE4)


def _canonical_morph(segs, tris):
    """The ids of the morph's segments follow the slots of a hash table filled by atomics: they differ from run to run (the only arrays
    here that do).  Canonical form: the segments as sorted rows of point ids; every triangle as its three segments' point pairs in the
    cyclic order it has, turned so that the smallest pair comes first; the triangles' rows sorted."""
    segs, tris = np.asarray(segs, dtype=np.int64).reshape(-1, 2), np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    assert len(tris) == 0 or (tris.min() >= 0 and tris.max() < len(segs))
    seg_id = segs[:, 0] * (segs.max() + 1 if len(segs) else 1) + segs[:, 1]
    t = seg_id[tris]                                               # one number per segment that does not depend on its id
    first = np.argmin(t, axis=1)
    t = np.stack([np.take_along_axis(t, ((first + s) % 3)[:, None], axis=1)[:, 0] for s in range(3)], axis=1)
    return np.sort(seg_id), t[np.lexsort(t.T[::-1])]


def produce(name):
    "-> (context, the counts dict the producer returned or None, extra arrays of a 4-D producer)"
    from contourist_amd import _ffi
    ctx, c = fresh3()
    corner = np.array(SHAPE3) - 1
    out, extra = None, {}
    if name == "postprocess3d":
        out = ctx.postprocess3d(0)
    elif name == "postprocess3d_noclean":
        out = ctx.postprocess3d(1)
    elif name == "capped":
        ctx.cap3d("all", "above")
        out = ctx.postprocess3d_capped(0)
    elif name == "mesh":
        out = ctx.postprocess3d_mesh(inputs()["mesh"][0], inputs()["mesh"][1], corner, flags=_ffi.CX_MESH_OF_THE_MARCH)
    elif name in ("shard_begin", "shard_finish"):
        L = ctx.shard_begin(0, SHAPE3[0] - 1)
        out = dict(L["counts"], n_own_lower=L["n_own_lower"], n_upper_copies=L["n_upper_copies"], n_candidates=len(L["cand_label"]))
        if name == "shard_finish":
            out = ctx.shard_finish([], [])
    elif name in ("simplify", "simplify_dry", "simplify_normals"):
        ctx.postprocess3d(0)
        out = ctx.level1_simplify(2.0, {"simplify": 0, "simplify_dry": _ffi.CX_SIMPLIFY_COUNT_ONLY, "simplify_normals": _ffi.CX_SIMPLIFY_NORMALS}[name])
    elif name == "clip_plane":
        ctx.postprocess3d(0)
        out = ctx.level1_clip_plane((0.0, 0.0, 1.0), 3.3)
    elif name in ("keep_subset", "keep_all"):
        p = ctx.postprocess3d(0)
        assert p["n_components"] == 3
        out = ctx.level1_keep_components([1, 0, 1] if name == "keep_subset" else [1, 1, 1])
    elif name == "surface_geometry":
        ctx.postprocess3d(0)
        pts, tris = ctx.surface_geometry(inputs()["level1"][0], inputs()["level1"][1], True)
        extra = dict(sg_points=pts, sg_triangles=tris)
    elif name == "level0_points":
        ctx.postprocess3d(0)
        extra = dict(points0=ctx.level0_points_f64(c))
    elif name == "extract3d":
        ctx.postprocess3d(0)
        ctx.extract3d(0.25)
    elif name in PRODUCERS_4D:
        ctx.postprocess3d(0)
        march4(ctx)
        out = ctx.postprocess4d(100)
        pts4, tets = ctx.download_level1_4d(out)
        extra = dict(points4=pts4, tets=tets)
        if name == "morph_triangles":
            mp, ms, mt, ncomp = ctx.morph_triangles()
            ms, mt = _canonical_morph(ms, mt)
            extra.update(morph_points=mp, morph_segments=ms, morph_triangles=mt)
            out = dict(out, n_morph_components=ncomp)
    else:
        raise KeyError(name)
    return ctx, out, extra


def read(ctx, reader, tmpdir, bufs):
    "one reader through the C ABI, into host buffers with room for ROOM rows whatever the state holds -> the class of its return"
    L, h = ctx.lib, ctx.handle
    f64, i32 = bufs["f64"], bufs["i32"]
    p1, p2, n1, n2 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int64(0)
    if reader == "download":
        rc = L.cx_level1_download(h, f64.ctypes.data, i32.ctypes.data)
    elif reader == "keys":
        rc = L.cx_level1_download_keys(h, i32.ctypes.data)
    elif reader == "device_ptrs":
        rc = L.cx_level1_device_ptrs(h, ctypes.byref(p1), ctypes.byref(p2), ctypes.byref(n1), ctypes.byref(n2))
    elif reader == "write":
        rc = L.cx_level1_write(h, 0, os.fsencode(os.path.join(tmpdir, "mesh.ply")), None, f64.ctypes.data)
    elif reader == "normals":
        rc = L.cx_level1_normals_download(h, None, f64.ctypes.data)
    elif reader == "curvature":
        rc = L.cx_level1_curvature_download(h, None, f64.ctypes.data)
    elif reader == "sample":
        rc = L.cx_level1_sample_grid(h, bufs["grid"].ctypes.data, 0, 0, ctypes.byref(p1), f64.ctypes.data)
    elif reader == "components":
        rc = L.cx_level1_components(h, None, ctypes.byref(n1), None, f64.ctypes.data)
    elif reader == "component_labels":
        rc = L.cx_level1_component_labels_download(h, i32.ctypes.data, bufs["i32b"].ctypes.data)
    elif reader == "topology":
        rc = L.cx_level1_topology(h, ctypes.byref(n1), ctypes.byref(p1))
    elif reader == "simplify_map":
        rc = L.cx_level1_simplify_map_download(h, i32.ctypes.data)
    elif reader == "clip_map":
        rc = L.cx_level1_clip_map_download(h, i32.ctypes.data, f64.ctypes.data)
    elif reader == "download_4d":
        rc = L.cx_level1_4d_download(h, f64.ctypes.data, i32.ctypes.data)
    else:
        raise KeyError(reader)
    return _cls(rc)


def walk(name, tmpdir, skip_cross=False):
    """producer `name` on a fresh context, then every reader -> dict(readers, counts, sha, bytes).  skip_cross: the readers of the 3-D
    mesh are not called after a 4-D producer (None in their place): for recording on a commit where they read out of bounds."""
    from contourist_amd import _ffi
    ctx, out, extra = produce(name)
    bufs = dict(f64=np.zeros(ROOM * 4, np.float64), i32=np.zeros(ROOM * 4, np.int32), i32b=np.zeros(ROOM, np.int32), grid=field3())
    sha = {k: _sha(v) for k, v in sorted(extra.items())}
    res = {}
    for r in READERS:
        cross = name in PRODUCERS_4D and r != "download_4d"
        res[r] = None if (cross and skip_cross) else read(ctx, r, str(tmpdir), bufs)
        if r == "device_ptrs" and res[r] == "OK" and res["download"] == "OK" and res["keys"] == "OK" and name not in PRODUCERS_4D:
            _p, _t, nv, nt = ctx.level1_device_ptrs()
            pts, tris = ctx.download_level1(dict(n_vertices=nv, n_triangles=nt))
            keys = ctx.download_level1_keys(dict(n_vertices=nv))
            sha.update(points=_sha(pts), triangles=_sha(tris), keys=_sha(keys), n=(nv, nt))
    live = _ffi.device_bytes(ctx.handle)
    ctx.close()
    return dict(readers=tuple(res[r] for r in READERS), counts=out, sha=sha, bytes=live)


# ---- recorded on the parent commit (see the module's docstring) -------------------------------------------------------------------------
RECORDED = {'postprocess3d': {'readers': ('OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
                   'counts': {'n_vertices': 1065, 'n_triangles': 2032, 'n_after_weld': 2032, 'n_after_tiny': 2032, 'n_components': 3},
                   'sha': {'points': 'cfa83654cf46b579', 'triangles': '87b782288e4fcaa7', 'keys': 'a991bb242863b56d', 'n': (1065, 2032)},
                   'bytes': (1847833, 83)},
 'postprocess3d_noclean': {'readers': ('OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
                           'counts': {'n_vertices': 1065, 'n_triangles': 2032, 'n_after_weld': 2032, 'n_after_tiny': 2032, 'n_components': 3},
                           'sha': {'points': 'cfa83654cf46b579', 'triangles': '87b782288e4fcaa7', 'keys': 'a991bb242863b56d', 'n': (1065, 2032)},
                           'bytes': (1847833, 83)},
 'capped': {'readers': ('OK', 'OK', 'OK', 'OK', 'UNSUPPORTED', 'UNSUPPORTED', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
            'counts': {'n_vertices': 1604, 'n_triangles': 3196, 'n_after_weld': 3196, 'n_after_tiny': 3196, 'n_components': 3},
            'sha': {'points': '9a8504e9188bce37', 'triangles': '3db191154704c0d0', 'keys': '393a03a774d2de57', 'n': (1604, 3196)},
            'bytes': (2089861, 72)},
 'mesh': {'readers': ('OK', 'OK', 'OK', 'OK', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
          'counts': {'n_vertices': 1065, 'n_triangles': 2032, 'n_after_weld': 2032, 'n_after_tiny': 2032, 'n_components': 3},
          'sha': {'points': '1abf49c20db951bb', 'triangles': 'c45b3bd32a3ef018', 'keys': '563df92d2b107552', 'n': (1065, 2032)},
          'bytes': (1760672, 77)},
 'shard_begin': {'readers': ('STATE', 'STATE', 'STATE', 'STATE', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'STATE', 'STATE', 'STATE'),
                 'counts': {'n_after_weld': 2032, 'n_after_tiny': 2032, 'n_own_lower': 0, 'n_upper_copies': 0, 'n_candidates': 0},
                 'sha': {},
                 'bytes': (1570500, 39)},
 'shard_finish': {'readers': ('OK', 'OK', 'OK', 'OK', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'STATE',
                              'STATE', 'STATE'),
                  'counts': {'n_vertices': 1065, 'n_triangles': 2032, 'n_components': 3},
                  'sha': {'points': 'cfa83654cf46b579', 'triangles': '87b782288e4fcaa7', 'keys': 'a991bb242863b56d', 'n': (1065, 2032)},
                  'bytes': (1574764, 41)},
 'simplify': {'readers': ('OK', 'OK', 'OK', 'OK', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE'),
              'counts': {'n_vertices': 95,
                         'n_triangles': 156,
                         'n_components': 3,
                         'n_clusters': 95,
                         'cell': (2.0, 2.0, 2.0),
                         'clamped': 0,
                         'n_distinct': 160,
                         'q': 48},
              'sha': {'points': '3e1595b1e1c4d6aa', 'triangles': '04a8a94060b8e015', 'keys': '42029a6199f6fa63', 'n': (95, 156)},
              'bytes': (1672412, 86)},
 'simplify_dry': {'readers': ('OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
                  'counts': {'n_vertices': 0,
                             'n_triangles': 0,
                             'n_components': 0,
                             'n_clusters': 95,
                             'cell': (2.0, 2.0, 2.0),
                             'clamped': 0,
                             'n_distinct': 160,
                             'q': 48},
                  'sha': {'points': 'cfa83654cf46b579', 'triangles': '87b782288e4fcaa7', 'keys': 'a991bb242863b56d', 'n': (1065, 2032)},
                  'bytes': (1910089, 90)},
 'simplify_normals': {'readers': ('OK', 'OK', 'OK', 'OK', 'OK', 'UNSUPPORTED', 'UNSUPPORTED', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE'),
                      'counts': {'n_vertices': 95,
                                 'n_triangles': 156,
                                 'n_components': 3,
                                 'n_clusters': 95,
                                 'cell': (2.0, 2.0, 2.0),
                                 'clamped': 0,
                                 'n_distinct': 160,
                                 'q': 48},
                      'sha': {'points': '3e1595b1e1c4d6aa', 'triangles': '04a8a94060b8e015', 'keys': '42029a6199f6fa63', 'n': (95, 156)},
                      'bytes': (1749181, 91)},
 'clip_plane': {'readers': ('OK', 'OK', 'OK', 'OK', 'UNSUPPORTED', 'UNSUPPORTED', 'UNSUPPORTED', 'OK', 'OK', 'OK', 'STATE', 'OK', 'STATE'),
                'counts': {'n_vertices': 970,
                           'n_triangles': 1724,
                           'n_components': 3,
                           'n_cut_vertices': 122,
                           'n_cut_triangles': 122,
                           'n_nonfinite': 0,
                           'n_on_cut': 0,
                           'n_raw_triangles': 1724},
                'sha': {'points': 'ba5ad3076a655070', 'triangles': '74b3a6d471728845', 'keys': 'd0e9b2f553ebeef3', 'n': (970, 1724)},
                'bytes': (1910772, 100)},
 'keep_subset': {'readers': ('OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
                 'counts': {'n_vertices': 829, 'n_triangles': 1564, 'n_components': 2},
                 'sha': {'points': '77fd98bacc21b96a', 'triangles': '6e2ef70fdefe3736', 'keys': '9f5b9d73317f772b', 'n': (829, 1564)},
                 'bytes': (1814344, 88)},
 'keep_all': {'readers': ('OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'OK', 'STATE', 'STATE', 'STATE'),
              'counts': {'n_vertices': 1065, 'n_triangles': 2032, 'n_components': 3},
              'sha': {'points': 'cfa83654cf46b579', 'triangles': '87b782288e4fcaa7', 'keys': 'a991bb242863b56d', 'n': (1065, 2032)},
              'bytes': (1847833, 83)},
 'surface_geometry': {'readers': ('STATE', 'STATE', 'STATE', 'STATE', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'STATE', 'STATE',
                                  'STATE'),
                      'counts': None,
                      'sha': {'sg_points': 'cfa83654cf46b579', 'sg_triangles': '87b782288e4fcaa7'},
                      'bytes': (1654300, 37)},
 'level0_points': {'readers': ('STATE', 'STATE', 'STATE', 'STATE', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'STATE', 'STATE', 'STATE'),
                   'counts': None,
                   'sha': {'points0': 'cfa83654cf46b579'},
                   'bytes': (1555996, 36)},
 'extract3d': {'readers': ('STATE', 'STATE', 'STATE', 'STATE', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'INVALID', 'STATE', 'STATE', 'STATE'),
               'counts': None,
               'sha': {},
               'bytes': (1555996, 36)},
 'postprocess4d': {'readers': (None, None, None, None, None, None, None, None, None, None, None, None, 'OK'),
                   'counts': {'n_vertices': 828, 'n_tetrahedra': 4662, 'n_after_drop': 4662, 'n_after_tiny': 4662},
                   'sha': {'points4': 'b29193df1874dcb0', 'tets': '10dc29918faf101f'},
                   'bytes': (2039234, 52)},
 'morph_triangles': {'readers': (None, None, None, None, None, None, None, None, None, None, None, None, 'OK'),
                     'counts': {'n_vertices': 828, 'n_tetrahedra': 4662, 'n_after_drop': 4662, 'n_after_tiny': 4662, 'n_morph_components': 4},
                     'sha': {'morph_points': 'b29193df1874dcb0',
                             'morph_segments': '8266d1ad65ee50e6',
                             'morph_triangles': '0872912a6ec7d454',
                             'points4': 'b29193df1874dcb0',
                             'tets': '10dc29918faf101f'},
                     'bytes': (4967418, 66)}}


def expected(name):
    E = dict(RECORDED[name])
    E["readers"] = tuple("STATE" if c is None else c for c in E["readers"])
    return E


_walked = {}


def walked(name, tmp_path_factory):
    if name not in _walked:
        _walked[name] = walk(name, tmp_path_factory.mktemp(name))
    return _walked[name]


@pytest.mark.parametrize("name", PRODUCERS)
def test_transition_matrix(name, tmp_path_factory):
    got = walked(name, tmp_path_factory)
    print(name, dict(zip(READERS, got["readers"])))
    assert dict(zip(READERS, got["readers"])) == dict(zip(READERS, expected(name)["readers"]))
    if name in PRODUCERS_4D:      # a reader of the 3-D mesh after a 4-D post-pass refuses, and the other way round
        assert all(c == "STATE" for r, c in zip(READERS, got["readers"]) if r != "download_4d")
    else:
        assert got["readers"][READERS.index("download_4d")] == "STATE"


@pytest.mark.parametrize("name", PRODUCERS)
def test_same_results(name, tmp_path_factory):
    got, E = walked(name, tmp_path_factory), expected(name)
    print(name, got["counts"], got["sha"], got["bytes"])
    assert got["counts"] == E["counts"]
    assert got["sha"] == E["sha"]
    assert tuple(got["bytes"]) == tuple(E["bytes"])


def _mesh_bytes(ctx, p):
    pts, tris = ctx.download_level1(p)
    return pts.tobytes(), tris.tobytes(), ctx.download_level1_keys(p).tobytes()


def test_refused_mesh_leaves_the_resident_mesh_alone():
    from contourist_amd import _ffi
    ctx, _c = fresh3()
    p = ctx.postprocess3d(0)
    before = _mesh_bytes(ctx, p)
    pts, tris = inputs()["mesh"]
    bad = tris.copy()
    bad[len(bad) // 2, 1] = len(pts)                      # one index past the last vertex
    with pytest.raises(_ffi.CxError) as e:
        ctx.postprocess3d_mesh(pts, bad, np.array(SHAPE3) - 1)
    assert e.value.code == _ffi.CX_ERR_INVALID
    assert _mesh_bytes(ctx, p) == before
    ctx.close()


def test_dry_run_simplify_leaves_the_resident_mesh_alone():
    from contourist_amd import _ffi
    ctx, _c = fresh3()
    p = ctx.postprocess3d(0)
    before = _mesh_bytes(ctx, p)
    gen_view = ctx.level1_components()
    d = ctx.level1_simplify(2.0, _ffi.CX_SIMPLIFY_COUNT_ONLY)
    assert d["n_clusters"] > 0
    assert _mesh_bytes(ctx, p) == before
    assert ctx.level1_components().tobytes() == gen_view.tobytes()
    assert len(ctx.level1_normals(p)) == p["n_vertices"]  # still the march's own mesh: edge ids, orientation tables
    ctx.close()
