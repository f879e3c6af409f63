"""Host: the restated seeded search of oracle/seeds.py itself -- its vectorised border test against the scalar one, its boxed 4-D
search against the reference's own surface voxels (tests/golden4d/reference_*_seeded.npz, rim voxels included), the
search without the shared visited set, the strict border rule and the group count.  No GPU."""
import os

import numpy as np
import pytest

import seeded_cases as sc
from conftest import ROOT
from oracle import seeds

G4 = os.path.join(ROOT, "tests", "golden4d")


def _field(dim):
    return sc.field3d() if dim == 3 else sc.field4d()


@pytest.mark.parametrize("dim", (3, 4))
def test_fields_are_what_the_gpu_tests_need(dim):
    A, v = _field(dim)
    sizes = sc.assert_preconditions(A, v)
    assert sizes == ([1416, 1306, 1036, 194] if dim == 3 else [1238, 1032, 102])
    P = sc.PAIRS3 if dim == 3 else sc.PAIRS4
    for n, pair in P.items():       # every far-apart pair reaches the one component it is named after, in either order
        assert len(seeds.reached(A, v, [pair])) == n and seeds.reached(A, v, [sc.flipped(pair)]) == seeds.reached(A, v, [pair])
        low, high = (np.array(p) for p in pair)
        assert np.abs(low - high).max() >= 8      # three bisection steps at least


@pytest.mark.parametrize("dim", (3, 4))
@pytest.mark.parametrize("strict", (False, True))
def test_vectorised_border_test_equals_the_scalar_one(dim, strict):
    A, v = _field(dim)
    mask = seeds.border_mask(A, v, strict)
    assert mask.shape == tuple(n - 1 for n in A.shape)
    rng = np.random.RandomState(5 + dim)
    on = np.argwhere(mask)
    some = np.concatenate([on[rng.choice(len(on), 300, replace=False)],
                           np.stack([rng.randint(-1, n + 1, size=600) for n in A.shape], axis=1)])     # (beyond the array too)
    look = seeds._border_test(A, v, strict, True)
    n_true = 0
    for p in some:
        p = tuple(int(x) for x in p)
        want = seeds.border_voxel(A, v, p, strict)
        assert look(p) == want, p
        n_true += want
    assert 300 <= n_true < len(some)


@pytest.mark.parametrize("dim", (3, 4))
def test_vectorised_search_equals_the_scalar_one(dim):
    "the whole search, bisection and growth, on the smallest component and inside a box on a large one"
    A, v = _field(dim)
    P = sc.PAIRS3 if dim == 3 else sc.PAIRS4
    small, big = (194, 1416) if dim == 3 else (102, 1238)
    lo, hi = ((20, 20, 5), (30, 38, 20)) if dim == 3 else ((7, 8, 7, 2), (12, 15, 12, 5))
    for eps, box in (([P[small]], (None, None)), ([P[big]], (lo, hi))):
        fast = seeds.reached(A, v, eps, *box)
        assert fast == seeds.reached(A, v, eps, *box, vectorised=False) and len(fast) > 50
    assert len(seeds.reached(A, v, [P[big]], lo, hi)) < big


def test_boxed_search_4d_equals_the_reference_on_its_own_demo():
    """the reference's test0 call (explicit end points, two start voxels outside the grid): the field sampled with a rim of one
    sample, the grid's box -- the oracle's hyper-voxels are the reference's, rim voxels included"""
    from oracle.make_goldens4d import test0_field, TEST0_END_POINTS
    G = np.load(os.path.join(G4, "reference_test0_seeded.npz"))
    g = np.arange(-1, 10, dtype=np.float64)
    A = test0_field(*np.meshgrid(g, g, g, g, indexing="ij"))
    eps = np.array(TEST0_END_POINTS) + 1
    surf = seeds.reached(A, float(G["value"]), eps, (1,) * 4, (9,) * 4)
    got = np.array(sorted(surf)) - 1
    sv = G["surface_voxels"]
    assert np.array_equal(got, sv[np.lexsort(sv.T[::-1])])
    assert int(((sv < 0) | (sv >= 8)).any(axis=1).sum()) > 0                                   # some of them in the rim
    # and through select4d: the mask over the oracle's tetrahedra keeps as many as the reference emitted
    M = sc.OracleMesh(A.astype(np.float32), float(G["value"]))            # (the march reads fp32 samples: same voxels here)
    keep, surf2 = seeds.select4d(M.A, M.value, eps, M.keys, M.cells, (1,) * 4, (9,) * 4)
    assert surf2 == surf and int(keep.sum()) == len(G["l0_tets"])
    whole, _ = seeds.select4d(M.A, M.value, eps, M.keys, M.cells)                              # without the box: more
    assert int(whole.sum()) > int(keep.sum())


def test_all_in_range_4d_equals_the_reference_on_an_open_surface():
    """the reference's exhaustive search on a surface that leaves the grid (every crossing segment a seed): every hyper-voxel of
    the grid's box and the start voxels in the rim"""
    from oracle.make_goldens4d import open_rim_field, OPEN_RIM
    G = np.load(os.path.join(G4, "reference_open_rim_seeded.npz"))
    gd = tuple(int(n) for n in G["grid_dimensions"])
    ax = [np.arange(-1, n + 2, dtype=np.float64) for n in gd]
    A = open_rim_field(*np.meshgrid(*ax, indexing="ij"))
    v = float(OPEN_RIM["value"])
    inner = A[tuple(slice(1, n + 2) for n in gd)]
    segs = sc.reference_crossing_segments(inner, gd, v)
    eps = np.array(segs) + 1
    hi = tuple(n + 1 for n in gd)
    surf = seeds.reached(A, v, eps, (1,) * 4, hi, all_in_range=True)
    sv = G["surface_voxels"]
    assert np.array_equal(np.array(sorted(surf)) - 1, sv[np.lexsort(sv.T[::-1])])
    assert int(((sv < 0) | (sv >= np.array(gd))).any(axis=1).sum()) == 109
    # the growth alone gives the same here (every group of the box has a seed) and the box alone does not (no rim voxels)
    assert seeds.reached(A, v, eps, (1,) * 4, hi) == surf
    assert len(seeds.reached(A, v, [], (1,) * 4, hi, all_in_range=True)) == len(surf) - 109


@pytest.mark.parametrize("dim", (3, 4))
def test_search_without_the_shared_visited_set(dim):
    A, v = _field(dim)
    P = sc.PAIRS3 if dim == 3 else sc.PAIRS4
    eps = list(P.values()) + [sc.flipped(p) for p in P.values()]
    assert seeds.initial_voxels(A, v, eps, shared_visited=False) == seeds.initial_voxels(A, v, eps)       # no two pairs collide
    many = eps * 9000                                                  # deduplicated first: costs nothing
    assert seeds.initial_voxels(A, v, many, shared_visited=False) == seeds.initial_voxels(A, v, eps)
    # two pairs whose high points' own voxels are not border voxels and share candidates: the second pair finds the first one's
    # voxel visited and moves on to the next candidate; without the set it takes the same voxel again
    eps = sc.COLLIDING3 if dim == 3 else sc.COLLIDING4
    seq, par = seeds.initial_voxels(A, v, eps), seeds.initial_voxels(A, v, eps, shared_visited=False)
    assert par < seq and len(seq) == len(par) + 1


@pytest.mark.parametrize("dim", (3, 4))
def test_strict_rule_and_groups_on_the_bridge_field(dim):
    A, v, pair = sc.bridge_field(dim)
    assert int((A == v).sum()) == 1
    loose, strict = seeds.reached(A, v, [pair]), seeds.reached(A, v, [pair], strict=True)
    assert strict < loose
    assert seeds.groups(A, v, strict, strict=True) == [(len(strict), len(strict)), (len(strict), 0)]      # two equal cubes, one kept
    assert len(seeds.groups(A, v, loose)) == 1 and len(loose) == 2 * len(strict) + 2 ** dim              # bridged by 2^dim voxels
    assert seeds.groups_kept(A, v, strict, strict=True) == 1


def test_groups_and_all_in_range_in_a_box():
    A, v = sc.field3d()
    rod = ((0, 9, 9), (40, 14, 14))                 # through the first sphere along axis 0: two caps inside the box
    eps = [[(11, 11, 11), (0, 11, 11)]]
    kept = seeds.reached(A, v, eps, *rod)
    assert seeds.groups(A, v, kept, *rod) == [(34, 0), (25, 25)]
    assert seeds.groups_kept(A, v, kept, *rod) == 1
    everything = seeds.reached(A, v, eps, *rod, all_in_range=True)
    assert everything == seeds.in_box_surface(A, v, *rod) and len(everything) == 59
    assert seeds.reached(A, v, [], *rod) == set() and seeds.reached(A, v, [], *rod, all_in_range=True) == everything
    assert seeds.in_box_surface(A, v, (5, 5, 20), (30, 30, 20)) == set()                                  # an empty box
    assert seeds.in_box_surface(A, v, (-3, -1, -9), (99, 41, 50)) == seeds.in_box_surface(A, v)           # clamped
