"""GPU: seeded selection of surface components (tetrahedral.py:396-463) -- the reference's own unit test run
verbatim through the mirrored API, and device == oracle on multi-component fields."""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu


def two_dots(x, y, z):
    if x == y == z == -8 or x == y == z == 0:
        return 1
    return -1


def test_reference_unit_test_verbatim():
    """contourist/test/test_tetrahedral.py:13-37, only the import changed"""
    from contourist_amd import tetrahedral
    f = two_dots
    mins = [-8] * 3
    maxes = [8] * 3
    deltas = [2] * 3
    eps = [[(-8, -8, -8), (-8, -8, 8)]]
    S = tetrahedral.TriangulatedIsosurfaces(mins, maxes, deltas, f, 0, eps)
    (points, triangles) = S.get_points_and_triangles()
    points = [tuple(int(i) for i in pt) for pt in points]
    triangle_vertices = set(frozenset(points[i] for i in triangle) for triangle in triangles)
    expected = set([frozenset([(-9, -9, -8), (-9, -8, -8), (-8, -8, -7)]),
                    frozenset([(-7, -8, -8), (-7, -8, -7), (-7, -7, -7)]),
                    frozenset([(-8, -8, -7), (-8, -7, -7), (-7, -7, -7)]),
                    frozenset([(-8, -8, -7), (-7, -8, -7), (-7, -7, -7)]),
                    frozenset([(-9, -9, -8), (-8, -9, -8), (-8, -8, -7)]),
                    frozenset([(-8, -7, -8), (-7, -7, -8), (-7, -7, -7)]),
                    frozenset([(-7, -8, -8), (-7, -7, -8), (-7, -7, -7)]),
                    frozenset([(-8, -7, -8), (-8, -7, -7), (-7, -7, -7)])])
    assert triangle_vertices == expected
    # and the golden written by the real reference for the same call
    G = np.load(os.path.join(GOLDEN_DIR, "two_dots.npz"))
    ref = set(frozenset(tuple(int(x) for x in G["l1_points"][i]) for i in t) for t in G["l1_triangles"])
    assert triangle_vertices == ref


def level0_on_device(A, v):
    from contourist_amd import _ffi
    ctx = _ffi.Context(0)
    ctx.upload_grid(A)
    counts = ctx.extract3d(v, _ffi.CX_DIAG_CPYTHON310)
    xyz, keys, tris = ctx.download_level0(counts)
    return ctx, counts, xyz, keys.astype(np.int64), tris.astype(np.int64)


@pytest.mark.parametrize("name,seed_sets", [("blobs27", 2), ("shells24", 2), ("noise24_v07", 3)])
def test_device_selection_equals_oracle(name, seed_sets):
    """seeds taken from crossing edges of individual components: the device keeps exactly the triangles the
    restated reference search keeps (fields without samples equal to the isovalue)"""
    from oracle import level0, seeds
    G = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    A, v = G["A"], float(G["value"])
    ctx, counts, xyz, keys, tris = level0_on_device(A, v)
    try:
        lin, d = keys >> 3, keys & 7
        n1n2 = A.shape[1] * A.shape[2]
        q = np.stack([lin // n1n2, (lin // A.shape[2]) % A.shape[1], lin % A.shape[2]], axis=1)
        dv = np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1)
        rng = np.random.RandomState(7)
        for trial in range(seed_sets):
            pick = rng.choice(len(keys), size=1 + trial, replace=False)
            eps = [[tuple(int(x) for x in q[p]), tuple(int(x) for x in q[p] + dv[p])] for p in pick]
            O = level0.march3d(A, v, diag_mode=1)
            ko = level0.edge_keys_from_pairs(O["pairs"], A.shape)
            want, _ = seeds.select(A, v, eps, ko, O["tris"])
            got = ctx.select_seeded(eps)
            assert got["triangles_kept"] == int(want.sum())
            # Level 1 of the selection == the oracle's Level 1 of the filtered Level-0 mesh (vertices of dropped
            # components do not exist for the weld)
            from oracle import postpass
            corner = np.array(A.shape) - 1
            used = np.zeros(len(ko), dtype=bool)
            used[O["tris"][want].ravel()] = True
            renum = np.cumsum(used) - 1
            L1 = postpass.level1_from_level0(ko[used], O["xyz"][used], renum[O["tris"][want]], corner)
            post = ctx.postprocess3d(0)
            pts, t1 = ctx.download_level1(post)
            assert post["n_after_weld"] == L1["n_after_weld"] and post["n_after_tiny"] == L1["n_after_tiny"]
            assert len(t1) == len(L1["triangles"])
            cmp = postpass.compare_level1(L1, pts, t1, corner, reach=0)
            assert not cmp["missing"] and not cmp["extra"] and not cmp["winding"]
    finally:
        ctx.close()


def test_bad_endpoints_are_rejected():
    from contourist_amd import _ffi
    G = np.load(os.path.join(GOLDEN_DIR, "sphere32.npz"))
    ctx, counts, xyz, keys, tris = level0_on_device(G["A"], float(G["value"]))
    try:
        with pytest.raises(_ffi.CxError):
            ctx.select_seeded([[(0, 0, 0), (0, 0, 1)]])          # both outside the sphere: do not straddle the isovalue
    finally:
        ctx.close()


def test_search_for_endpoints_with_skip():
    """skip > 1: the coarse crossing search seeds the growth; a component that the coarse lattice misses is not
    returned (the reference's sparsity mode, grid_field.py:64-84 + tetrahedral.py:396-463), a large one is."""
    from contourist_amd import tetrahedral
    n = 48
    ax = np.arange(n, dtype=np.float64)
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    big = np.sqrt((X - 16.3) ** 2 + (Y - 16.1) ** 2 + (Z - 16.2) ** 2) - 9.0       # sphere of radius 9
    small = np.sqrt((X - 38.5) ** 2 + (Y - 38.5) ** 2 + (Z - 38.5) ** 2) - 1.2     # sphere of radius 1.2 between coarse points
    A = np.minimum(big, small).astype(np.float32)
    full = tetrahedral.TriangulatedIsosurfaces([0] * 3, None, [1] * 3, A, 0.0, [])
    full.search_for_endpoints()
    p_all, t_all = full.get_points_and_triangles()
    coarse = tetrahedral.TriangulatedIsosurfaces([0] * 3, None, [1] * 3, A, 0.0, [])
    coarse.search_for_endpoints(skip=8)
    p_big, t_big = coarse.get_points_and_triangles()
    assert 0 < len(t_big) < len(t_all)
    assert np.all(np.linalg.norm(np.asarray(p_big) - np.array([16.3, 16.1, 16.2]), axis=1) < 10.5)   # only the big sphere
    near_small = np.linalg.norm(np.asarray(p_all) - 38.5, axis=1) < 3
    assert near_small.any()                                                            # the exhaustive search has both
    # closed surface: Euler characteristic 2
    assert len(p_big) - len(t_big) // 2 == 2


def test_many_seeds_take_the_parallel_path():
    """the one-thread-per-pair seed kernel (what more than 65 536 end point pairs get; forced here): same selection
    as the oracle on a field where every candidate voxel of a pair belongs to one component"""
    from oracle import level0, seeds
    G = np.load(os.path.join(GOLDEN_DIR, "blobs27.npz"))
    A, v = G["A"], float(G["value"])
    ctx, counts, xyz, keys, tris = level0_on_device(A, v)
    try:
        O = level0.march3d(A, v, diag_mode=1)
        ko = level0.edge_keys_from_pairs(O["pairs"], A.shape)
        lin, d = keys >> 3, keys & 7
        n1n2 = A.shape[1] * A.shape[2]
        q = np.stack([lin // n1n2, (lin // A.shape[2]) % A.shape[1], lin % A.shape[2]], axis=1)
        dv = np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1)
        # all crossing edges of the component that contains vertex 0, repeated to exceed 1024 pairs
        mask0, surf = seeds.select(A, v, [[tuple(q[0]), tuple(q[0] + dv[0])]], ko, O["tris"])
        vox = seeds.triangle_voxels(ko, O["tris"], A.shape)
        comp_vertices = np.unique(np.vectorize({int(k): n for n, k in enumerate(keys)}.get)(ko[np.unique(O["tris"][mask0])]))
        eps = [[tuple(int(x) for x in q[p]), tuple(int(x) for x in q[p] + dv[p])] for p in comp_vertices]
        while len(eps) <= 1024:
            eps = eps + eps
        got = ctx.select_seeded(eps, parallel=True)
        assert got["triangles_kept"] == int(mask0.sum())
    finally:
        ctx.close()


# ---- the selection against the restated search, boxes and all (fields, cases and the comparison: tests/seeded_cases.py) ----------
# Every comparison is exact: kept triangles as sets of sorted edge-key triples, triangles_kept, the vertex mask == used by a kept
# triangle, groups_kept and the seed kernel that ran (seeded_cases.run_case).

def _field3():
    import seeded_cases as sc
    A, v = sc.field3d()
    sc.assert_preconditions(A, v)            # no sample on the isovalue, >= 3 components, >= 2 of them across record blocks
    return sc, A, v, sc.oracle_mesh(A, v)


def _kept_sizes(r):
    return sorted(n for n, k in r["groups"] if k)


CUT6 = ((0, 0, 0), (6, 38, 41))              # the seed voxels of COLLIDING3 lie just outside: kept one by one, growing into one cap
FULL3 = ((-3, -1, -9), (99, 41, 50))        # beyond the array on both sides: clamped, equals the default
SHAPE3 = (40, 38, 41)


@pytest.mark.parametrize("which", [(1306,), (1416,), (1036,), (194,), (1306, 194), (1416, 1036)])
def test_components_from_far_end_points(which):
    """far-apart end points (device bisection), some as (high, low), one pair twice: each component on its own and two together"""
    sc, A, v, M = _field3()
    eps = [sc.PAIRS3[n] if i % 2 == 0 else sc.flipped(sc.PAIRS3[n]) for i, n in enumerate(which)]
    if which[0] in (1416, 194):
        eps[0] = sc.flipped(eps[0])
    eps.append(eps[0])
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, sc.case(eps))
        assert _kept_sizes(r) == sorted(which) and len(r["surf"]) == sum(which)            # (the oracle: what the case is about)
        assert not r["mismatches"], r["mismatches"]
        assert r["got"]["groups_kept"] == len(which)
    finally:
        D.close()


BOXES3 = {
    "lo>0": dict(box=((6, 5, 7), SHAPE3), seeds=(1306, 1416), kept=2, fewer=True),
    "hi<corner": dict(box=((0, 0, 0), (30, 38, 41)), seeds=(1416,), kept=1, fewer=True),      # through the 1416 sphere
    "upper face": dict(box=((0, 0, 0), (36, 33, 19)), seeds=(1416,), kept=1, fewer=True),      # hi on the sphere's last voxels
    "rod": dict(box=((0, 9, 9), (40, 14, 14)), eps=[[(11, 11, 11), (0, 11, 11)]], kept=1, groups=[(34, 0), (25, 25)]),
    "beyond": dict(box=FULL3, seeds=(1306, 194), kept=2, same_as_default=True),
    "empty": dict(box=((5, 5, 20), (30, 30, 20)), seeds=(1306, 1036), kept=0, only_seeds=True),
    "rim": dict(box=((1, 1, 1), (38, 36, 39)), seeds=(1416, 1036, 194), kept=3),
}


@pytest.mark.parametrize("name", sorted(BOXES3))
def test_in_range_boxes(name):
    """voxel_range: lo > 0 on every axis, hi below the corner through a big sphere, a box that splits one sphere into two in-box
    pieces of which one is seeded, a box beyond the array, an empty box (only the seed voxels), the one-voxel-rim box"""
    from oracle import seeds
    sc, A, v, M = _field3()
    B = BOXES3[name]
    eps = B.get("eps") or [sc.PAIRS3[n] for n in B["seeds"]]
    c = sc.case(eps, B["box"])
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, c)
        # what the case is about, from the oracle
        free = seeds.reached(A, v, eps)
        assert sum(1 for n, k in r["groups"] if k) == B["kept"]
        if B.get("fewer"):
            assert r["surf"] < free and len(r["surf"]) > 100
        if B.get("groups"):
            assert r["groups"] == B["groups"]
        if B.get("same_as_default"):
            assert r["surf"] == free
        if B.get("only_seeds"):
            assert r["surf"] == seeds.initial_voxels(A, v, eps) and 0 < int(r["want"].sum()) < 60
        if name == "upper face":
            hi = np.array(B["box"][1])
            vox = np.array(sorted(r["surf"]))
            assert all((vox[:, a] == hi[a] - 1).any() for a in range(3))      # kept voxels on every upper face: hi - 1 is in
            assert all((np.array(sorted(free))[:, a] == hi[a]).any() for a in range(3))      # ... and hi itself is surface, left out
        assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


@pytest.mark.parametrize("all_in_range", (False, True))
@pytest.mark.parametrize("side", ("hi", "lo"))
def test_seed_voxels_outside_the_box(side, all_in_range):
    """the seed voxels lie one step outside the box: kept, and they grow one step into it.  With ALL_IN_RANGE every surface voxel
    of the box is kept as well, whatever its group."""
    from oracle import seeds
    sc, A, v, M = _field3()
    eps = [[(28, 27, 12), (39, 27, 12)]] if side == "hi" else [[(28, 27, 12), (0, 27, 12)]]
    start = np.array(sorted(seeds.initial_voxels(A, v, eps)))
    if side == "hi":
        box = ((0, 0, 0), (int(start[:, 0].min()), 38, 41))
    else:
        box = ((int(start[:, 0].max()) + 1, 0, 0), SHAPE3)
    c = sc.case(eps, box, all_in_range=all_in_range)
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, c)
        inside = seeds.in_box_surface(A, v, *box)
        assert len(start) == 2 and not (set(map(tuple, start.tolist())) & inside)       # both seed voxels outside the box
        assert set(map(tuple, start.tolist())) <= r["surf"]                              # kept all the same
        grown = r["surf"] & inside
        if all_in_range:
            assert grown == inside and len(r["groups"]) >= 2 and all(k == n for n, k in r["groups"])
            assert r["got"]["groups_kept"] == len(r["groups"])
        else:
            assert 100 < len(grown) < len(inside) and _kept_sizes(r) == [len(grown)]    # one in-box group, reached in one step
            assert r["got"]["groups_kept"] == 1
        assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_parallel_seed_kernel_where_the_choice_matters():
    """CX_SEED_PARALLEL against the oracle without the shared visited set, on pairs that collide (the sequential oracle picks
    another voxel there): with an empty box the kept triangles are exactly those of the seed voxels"""
    sc, A, v, M = _field3()
    empty = ((0, 0, 0), (0, 0, 0))
    for box in (empty, CUT6):
        ws, wp = M.select(sc.case(sc.COLLIDING3, box))[0], M.select(sc.case(sc.COLLIDING3, box, parallel=True))[0]
        assert int(wp.sum()) < int(ws.sum()) and not (wp & ~ws).any()                    # the two oracles differ here
    D = sc.DeviceMesh(A, v)
    try:
        for box in (empty, None, CUT6):
            seq, par = sc.case(sc.COLLIDING3, box), sc.case(sc.COLLIDING3, box, parallel=True)
            for c in (par, seq, par):
                r = sc.run_case(D, M, c)
                assert not r["mismatches"], (box, c["parallel"], r["mismatches"])
        r = sc.run_case(D, M, sc.case(list(sc.PAIRS3.values()), None, parallel=True))       # far-apart pairs bisected per thread
        assert _kept_sizes(r) == [194, 1036, 1306, 1416] and not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_more_than_65536_pairs_take_the_parallel_kernel_by_themselves():
    sc, A, v, M = _field3()
    short = sc.COLLIDING3 + [sc.PAIRS3[1036], sc.flipped(sc.PAIRS3[194])]
    eps = (short * (65537 // len(short) + 1))[:65537]
    c = sc.case(eps, CUT6)
    ws, wp = M.select(dict(c, eps=short))[0], M.select(dict(c, eps=short, parallel=True))[0]
    assert int(wp.sum()) < int(ws.sum())                                                 # the sequential kernel would keep more
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, dict(c, oracle=dict(shared_visited=False)))
        assert D.ctx.seeded_mode() == "parallel" and len(eps) == 65537
        assert np.array_equal(r["want"], wp) and not r["mismatches"], r["mismatches"]
        r = sc.run_case(D, M, sc.case(eps[:65536], c["box"]))                            # one fewer: the reference's order
        assert D.ctx.seeded_mode() == "sequential"
        assert np.array_equal(r["want"], ws) and not r["mismatches"], r["mismatches"]
    finally:
        D.close()


@pytest.mark.parametrize("name", ("uint8", "int16"))
def test_typed_grids_against_the_oracle(name):
    """8- and 16-bit samples read in their own type by the seed kernels: the mask equals the oracle's on the quantised values"""
    sc, A, v, _ = _field3()
    if name == "uint8":
        q, value = np.clip(np.round(128 + 4 * A.astype(np.float64)), 0, 255).astype(np.uint8), 128.5
    else:
        q, value = np.round(100 * A.astype(np.float64)).astype(np.int16), 0.5
    Q = q.astype(np.float64)
    sizes = sc.assert_preconditions(Q, value)
    M = sc.oracle_mesh(Q, value)
    D = sc.DeviceMesh(q, value, native=True)
    try:
        assert D.ctx.grid_info()["dtype"] == name
        eps = [sc.PAIRS3[1306], sc.flipped(sc.PAIRS3[194])]
        cut = ((0, 0, 0), (40, 14, 41))                       # through the larger of the two
        for c in (sc.case(eps), sc.case(eps, parallel=True), sc.case(eps, cut), sc.case(eps, cut, parallel=True)):
            r = sc.run_case(D, M, c)
            assert len(_kept_sizes(r)) == 2 and (c["box"] is None) == (_kept_sizes(r) == sorted([sizes[1], sizes[3]]))
            assert not r["mismatches"], (c["parallel"], r["mismatches"])
    finally:
        D.close()


def test_voxels_that_only_touch_the_isovalue_do_not_bridge_groups():
    """DESIGN.md's deviation: one sample equal to the isovalue among higher ones, between two blobs.  The reference's border_voxel
    bridges the groups (oracle, default rule: both blobs), the strict sign change does not (oracle, strict: one) -- the device
    keeps the strict one's triangles"""
    import seeded_cases as sc
    A, v, pair = sc.bridge_field(3)
    M = sc.oracle_mesh(A, v)
    loose, strict = M.select(sc.case([pair])), M.select(sc.case([pair], strict=True))
    assert int(loose[0].sum()) == 2 * int(strict[0].sum()) > 0 and strict[1] < loose[1]
    D = sc.DeviceMesh(A, v)
    try:
        for parallel in (False, True):
            r = sc.run_case(D, M, sc.case([pair], strict=True, parallel=parallel))
            assert np.array_equal(r["want"], strict[0]) and r["groups"] == [(len(strict[1]), len(strict[1])), (len(strict[1]), 0)]
            assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_no_end_points_and_an_empty_extraction():
    from contourist_amd import _ffi
    from oracle import seeds
    sc, A, v, M = _field3()
    D = sc.DeviceMesh(A, v)
    try:
        rod = BOXES3["rod"]["box"]
        r = sc.run_case(D, M, sc.case([]))
        assert not r["mismatches"] and r["got"] == dict(seed_voxels=0, groups_kept=0, triangles_kept=0, kept=0) and not r["mask"].any()
        r = sc.run_case(D, M, sc.case([], rod))
        assert not r["mismatches"] and r["got"]["triangles_kept"] == 0
        r = sc.run_case(D, M, sc.case([], rod, all_in_range=True))                       # exactly the voxels of the box
        assert r["surf"] == seeds.in_box_surface(A, v, *rod) and r["got"]["groups_kept"] == 2 and r["got"]["triangles_kept"] > 0
        assert not r["mismatches"], r["mismatches"]
        # an empty extraction: isovalue above every sample
        counts = D.ctx.extract3d(float(A.max()) + 1.0, _ffi.CX_DIAG_CPYTHON310)
        assert counts["n_triangles"] == 0 and counts["n_vertices"] == 0
        for flags in (dict(), dict(all_in_range=True), dict(parallel=True), dict(voxel_range=rod)):
            assert D.ctx.select_seeded([], **flags) == dict(seed_voxels=0, groups_kept=0, triangles_kept=0)
            tk, vk = D.ctx.seeded_masks(counts)
            assert len(tk) == 0 and len(vk) == 0
    finally:
        D.close()


def test_a_rejected_call_leaves_the_context_without_a_selection():
    from contourist_amd import _ffi
    sc, A, v, M = _field3()
    D = sc.DeviceMesh(A, v)
    try:
        good = sc.case([sc.PAIRS3[194]])
        outside = [[(30, 10, 30), (30, 10, 41)]]             # k = 41 is not in the array
        one_side = [[(0, 0, 0), (0, 37, 0)]]                 # both high
        assert A[0, 0, 0] > v and A[0, 37, 0] > v
        for bad in (outside, one_side, [sc.PAIRS3[1306]] + one_side, outside + [sc.PAIRS3[1306]]):
            for parallel in (False, True):
                r = sc.run_case(D, M, good)
                assert not r["mismatches"] and not r["mask"].all()
                with pytest.raises(_ffi.CxError) as e:
                    D.ctx.select_seeded(bad, parallel=parallel)
                assert e.value.code == -1
                tk, vk = D.ctx.seeded_masks(D.counts)        # no selection: everything
                assert tk.all() and vk.all() and len(tk) == D.counts["n_triangles"]
        r = sc.run_case(D, M, sc.case([sc.PAIRS3[1036]], BOXES3["lo>0"]["box"]))
        assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_one_context_sequential_parallel_boxes_and_a_4d_selection_in_between():
    """the scratch buffers (seed_buf) are shared by all of these: every call gives the oracle's mask"""
    sc, A, v, M = _field3()
    A4, v4 = sc.field4d()
    M4 = sc.oracle_mesh(A4, v4)
    D = sc.DeviceMesh(A, v)
    try:
        far = list(sc.PAIRS3.values())
        cases = [sc.case(far[:2]), sc.case(sc.COLLIDING3, BOXES3["empty"]["box"], parallel=True), sc.case(far[2:], BOXES3["rim"]["box"]),
                 sc.case(far[1:3], BOXES3["hi<corner"]["box"], parallel=True), sc.case([far[3]], BOXES3["lo>0"]["box"], all_in_range=True),
                 sc.case(far[:1])]
        for c in cases[:3]:
            r = sc.run_case(D, M, c)
            assert not r["mismatches"], r["mismatches"]
        D4 = sc.DeviceMesh(A4, v4, ctx=D.ctx)                # a 4-D extraction and selection on the same context
        r4 = sc.run_case(D4, M4, sc.case([sc.PAIRS4[1238]], ((1, 1, 1, 1), (12, 13, 12, 6))))
        assert not r4["mismatches"] and r4["got"]["tetrahedra_kept"] > 0, r4["mismatches"]
        for c in cases[3:]:
            r = sc.run_case(D, M, c)
            assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_level1_after_a_boxed_selection_with_a_seed_outside_the_box():
    """postprocess3d after a boxed selection == the oracle's Level 1 of the filtered Level-0 mesh (as
    test_device_selection_equals_oracle does without a box)"""
    from oracle import postpass, seeds
    sc, A, v, M = _field3()
    eps = [[(28, 27, 12), (39, 27, 12)], sc.PAIRS3[194]]
    start = np.array(sorted(seeds.initial_voxels(A, v, eps[:1])))
    box = ((0, 0, 0), (int(start[:, 0].min()), 38, 41))
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, sc.case(eps, box))
        assert not r["mismatches"], r["mismatches"]
        assert not (set(map(tuple, start.tolist())) & seeds.in_box_surface(A, v, *box)) and r["got"]["groups_kept"] == 2
        want, O, ko = r["want"], M.O, M.keys
        corner = np.array(A.shape) - 1
        used = np.zeros(len(ko), dtype=bool)
        used[O["tris"][want].ravel()] = True
        renum = np.cumsum(used) - 1
        L1 = postpass.level1_from_level0(ko[used], O["xyz"][used], renum[O["tris"][want]], corner)
        post = D.ctx.postprocess3d(0)
        pts, t1 = D.ctx.download_level1(post)
        assert post["n_after_weld"] == L1["n_after_weld"] and post["n_after_tiny"] == L1["n_after_tiny"]
        assert len(t1) == len(L1["triangles"]) > 0
        cmp = postpass.compare_level1(L1, pts, t1, corner, reach=0)
        assert not cmp["missing"] and not cmp["extra"] and not cmp["winding"]
    finally:
        D.close()
