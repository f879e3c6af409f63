"""GPU: the 4-D seeded selection (cx_seed4.hip, cx_select_seeded4d_ex) against the restated search of oracle/seeds.py, boxes and
all: kept tetrahedra as sets of sorted edge-key quadruples, tetrahedra_kept, groups_kept and the seed kernel that ran -- all exact
(fields, cases and the comparison: tests/seeded_cases.py; the 3-D counterpart: tests/test_gpu_seeded.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE4 = (14, 15, 14, 8)
CUT2 = ((2, 0, 0, 0), SHAPE4)               # the seed voxels of COLLIDING4 lie just outside: kept one by one, growing into one piece
BOXES4 = {
    "lo>0": dict(box=((2, 3, 2, 1), SHAPE4), seeds=(1032, 1238), kept=2, fewer=True),
    "hi<corner": dict(box=((0, 0, 0, 0), (10, 15, 14, 8)), seeds=(1238,), kept=1, fewer=True),      # through the 1238 sphere
    "upper face": dict(box=((0, 0, 0, 0), (12, 13, 12, 6)), seeds=(1238,), kept=1, fewer=True),      # hi on the sphere's last voxels
    "rod": dict(box=((0, 3, 3, 3), (14, 5, 5, 5)), eps=[[(4, 4, 4, 3), (0, 4, 4, 3)]], kept=1, groups=[(15, 0), (10, 10)]),
    "beyond": dict(box=((-3, -1, -9, -2), (99, 16, 20, 9)), seeds=(1032, 102), kept=2, same_as_default=True),
    "empty": dict(box=((2, 2, 2, 4), (12, 12, 12, 4)), seeds=(1032, 1238), kept=0, only_seeds=True),
    "rim": dict(box=((1, 1, 1, 1), (12, 13, 12, 6)), seeds=(1032, 1238, 102), kept=3),
}


def _field4():
    import seeded_cases as sc
    A, v = sc.field4d()
    sc.assert_preconditions(A, v)            # no sample on the isovalue, >= 3 components, >= 2 of them across record blocks
    return sc, A, v, sc.oracle_mesh(A, v)


def _kept_sizes(r):
    return sorted(n for n, k in r["groups"] if k)


@pytest.mark.parametrize("which", [(1032,), (1238,), (102,), (1032, 102), (1238, 1032)])
def test_components_from_far_end_points_4d(which):
    """far-apart end points (device bisection), some as (high, low), one pair twice: each component on its own and two together"""
    sc, A, v, M = _field4()
    eps = [sc.PAIRS4[n] if i % 2 == 0 else sc.flipped(sc.PAIRS4[n]) for i, n in enumerate(which)]
    if which[0] in (1238,):
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


@pytest.mark.parametrize("name", sorted(BOXES4))
def test_in_range_boxes_4d(name):
    """voxel_range: lo > 0 on every axis, hi below the corner through a big sphere, a box that splits one sphere into two in-box
    pieces of which one is seeded, a box beyond the array, an empty box (only the seed voxels), the one-voxel-rim box"""
    from oracle import seeds
    sc, A, v, M = _field4()
    B = BOXES4[name]
    eps = B.get("eps") or [sc.PAIRS4[n] for n in B["seeds"]]
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, sc.case(eps, B["box"]))
        free = seeds.reached(A, v, eps)
        assert sum(1 for n, k in r["groups"] if k) == B["kept"]
        if B.get("fewer"):
            assert r["surf"] < free and len(r["surf"]) > 100
        if B.get("groups"):
            assert r["groups"] == B["groups"]
        if B.get("same_as_default"):
            assert r["surf"] == free
        if B.get("only_seeds"):
            assert r["surf"] == seeds.initial_voxels(A, v, eps) and 0 < int(r["want"].sum()) < 400
        if name == "upper face":
            hi = np.array(B["box"][1])
            vox = np.array(sorted(r["surf"]))
            assert all((vox[:, a] == hi[a] - 1).any() for a in range(4))      # kept hyper-voxels on every upper face: hi - 1 is in
            assert all((np.array(sorted(free))[:, a] == hi[a]).any() for a in range(4))      # ... and hi itself is surface, left out
        assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


@pytest.mark.parametrize("all_in_range", (False, True))
@pytest.mark.parametrize("side", ("hi", "lo"))
def test_seed_voxels_outside_the_box_4d(side, all_in_range):
    """the seed voxels lie one step outside the box: kept, and they grow one step into it.  With ALL_IN_RANGE every surface
    hyper-voxel of the box is kept as well, whatever its group."""
    from oracle import seeds
    sc, A, v, M = _field4()
    if side == "hi":          # along axis 0, the box ends below the seed voxels
        eps = [[(10, 10, 10, 4), (13, 10, 10, 4)]]
        start = np.array(sorted(seeds.initial_voxels(A, v, eps)))
        box = ((0, 0, 0, 0), (int(start[:, 0].min()), 15, 14, 8))
    else:                     # along the last axis, the box begins above them
        eps = [[(10, 10, 10, 4), (10, 10, 10, 0)]]
        start = np.array(sorted(seeds.initial_voxels(A, v, eps)))
        box = ((0, 0, 0, int(start[:, 3].max()) + 1), SHAPE4)
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, sc.case(eps, box, all_in_range=all_in_range))
        inside = seeds.in_box_surface(A, v, *box)
        assert len(start) >= 1 and not (set(map(tuple, start.tolist())) & inside)       # the seed voxels are outside the box
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


def test_parallel_seed_kernel_where_the_choice_matters_4d():
    """CX_SEED_PARALLEL against the oracle without the shared visited set, on pairs that collide (the sequential oracle picks
    another hyper-voxel there): with an empty box the kept tetrahedra are exactly those of the seed voxels"""
    sc, A, v, M = _field4()
    empty = ((0, 0, 0, 0), (0, 0, 0, 0))
    for box in (empty, CUT2):
        ws, wp = M.select(sc.case(sc.COLLIDING4, box))[0], M.select(sc.case(sc.COLLIDING4, box, parallel=True))[0]
        assert int(wp.sum()) < int(ws.sum()) and not (wp & ~ws).any()                    # the two oracles differ here
    D = sc.DeviceMesh(A, v)
    try:
        for box in (empty, None, CUT2):
            seq, par = sc.case(sc.COLLIDING4, box), sc.case(sc.COLLIDING4, box, parallel=True)
            for c in (par, seq, par):
                r = sc.run_case(D, M, c)
                assert not r["mismatches"], (box, c["parallel"], r["mismatches"])
        r = sc.run_case(D, M, sc.case(list(sc.PAIRS4.values()), None, parallel=True))       # far-apart pairs bisected per thread
        assert _kept_sizes(r) == [102, 1032, 1238] and not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_more_than_16384_pairs_take_the_parallel_kernel_by_themselves():
    sc, A, v, M = _field4()
    short = sc.COLLIDING4 + [sc.PAIRS4[1238], sc.flipped(sc.PAIRS4[102])]
    eps = (short * (16385 // len(short) + 1))[:16385]
    c = sc.case(eps, CUT2)
    ws, wp = M.select(dict(c, eps=short))[0], M.select(dict(c, eps=short, parallel=True))[0]
    assert int(wp.sum()) < int(ws.sum())                                                 # the sequential kernel would keep more
    D = sc.DeviceMesh(A, v)
    try:
        r = sc.run_case(D, M, dict(c, oracle=dict(shared_visited=False)))
        assert D.ctx.seeded_mode() == "parallel" and len(eps) == 16385
        assert np.array_equal(r["want"], wp) and not r["mismatches"], r["mismatches"]
        r = sc.run_case(D, M, sc.case(eps[:16384], c["box"]))                            # one fewer: the reference's order
        assert D.ctx.seeded_mode() == "sequential"
        assert np.array_equal(r["want"], ws) and not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_voxels_that_only_touch_the_isovalue_do_not_bridge_groups_4d():
    """the deviation stated in cx_seed4.hip and DESIGN.md: one sample equal to the isovalue among higher ones, between two blobs.
    The reference's border_voxel bridges the groups (oracle, default rule: both blobs), the strict sign change does not (oracle,
    strict: one) -- the device keeps the strict one's tetrahedra"""
    import seeded_cases as sc
    A, v, pair = sc.bridge_field(4)
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


def test_no_end_points_and_an_empty_extraction_4d():
    from contourist_amd import _ffi
    from oracle import seeds
    sc, A, v, M = _field4()
    D = sc.DeviceMesh(A, v)
    try:
        rod = BOXES4["rod"]["box"]
        r = sc.run_case(D, M, sc.case([]))
        assert not r["mismatches"] and r["got"] == dict(seed_voxels=0, groups_kept=0, tetrahedra_kept=0, kept=0) and not r["mask"].any()
        r = sc.run_case(D, M, sc.case([], rod))
        assert not r["mismatches"] and r["got"]["tetrahedra_kept"] == 0
        r = sc.run_case(D, M, sc.case([], rod, all_in_range=True))                       # exactly the hyper-voxels of the box
        assert r["surf"] == seeds.in_box_surface(A, v, *rod) and r["got"]["groups_kept"] == 2 and r["got"]["tetrahedra_kept"] > 0
        assert not r["mismatches"], r["mismatches"]
        # an empty extraction: isovalue above every sample
        counts = D.ctx.extract4d(float(A.max()) + 1.0, _ffi.CX_DIAG_CPYTHON310)
        assert counts["n_tetrahedra"] == 0 and counts["n_vertices"] == 0
        for flags in (dict(), dict(all_in_range=True), dict(parallel=True), dict(voxel_range=rod)):
            assert D.ctx.select_seeded4d([], **flags) == dict(seed_voxels=0, groups_kept=0, tetrahedra_kept=0)
            assert len(D.ctx.seeded4d_mask(counts)) == 0
    finally:
        D.close()


def test_a_rejected_call_leaves_the_context_without_a_selection_4d():
    from contourist_amd import _ffi
    sc, A, v, M = _field4()
    D = sc.DeviceMesh(A, v)
    try:
        good = sc.case([sc.PAIRS4[102]])
        outside = [[(4, 11, 4, 6), (4, 11, 4, 8)]]           # l = 8 is not in the array
        one_side = [[(0, 0, 0, 0), (13, 0, 0, 0)]]           # both high
        assert A[0, 0, 0, 0] > v and A[13, 0, 0, 0] > v
        with pytest.raises(_ffi.CxError):                    # no selection yet
            D.ctx.seeded4d_mask(D.counts)
        for bad in (outside, one_side, [sc.PAIRS4[1032]] + one_side, outside + [sc.PAIRS4[1032]]):
            for parallel in (False, True):
                with pytest.raises(_ffi.CxError) as e:
                    D.ctx.select_seeded4d(bad, parallel=parallel)
                assert e.value.code == -1
                with pytest.raises(_ffi.CxError):            # ... and none after a rejected call, whatever came before
                    D.ctx.seeded4d_mask(D.counts)
                r = sc.run_case(D, M, good)
                assert not r["mismatches"] and not r["mask"].all(), r["mismatches"]
        r = sc.run_case(D, M, sc.case([sc.PAIRS4[1238]], BOXES4["lo>0"]["box"]))
        assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()


def test_one_context_sequential_parallel_and_boxes_4d():
    "the scratch buffers stay in the context between the calls: every call gives the oracle's mask"
    sc, A, v, M = _field4()
    D = sc.DeviceMesh(A, v)
    try:
        far = list(sc.PAIRS4.values())
        for c in (sc.case(far[:2]), sc.case(sc.COLLIDING4, BOXES4["empty"]["box"], parallel=True), sc.case(far[1:], BOXES4["rim"]["box"]),
                  sc.case(far[:2], BOXES4["hi<corner"]["box"], parallel=True), sc.case([far[2]], BOXES4["lo>0"]["box"], all_in_range=True),
                  sc.case(far[:1])):
            r = sc.run_case(D, M, c)
            assert not r["mismatches"], r["mismatches"]
    finally:
        D.close()
