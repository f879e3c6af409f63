"""CPU: the contract of cx_grid_watershed3d as tests/watershed_ref.py restates it from the header is well defined -- two computations of the
arrival cost agree, every region hangs together around its markers, every label attains the sample's minimax level -- with the hand-made
cases of the header's rules and the argument checks of contourist_amd.volume's helpers."""
import itertools

import numpy as np
import pytest

import recon_ref
import watershed_ref as W

CONNECTIVITIES = (1, 2, 3)


def random_case(seed, walls=True):
    "a tied uint8 relief below 255, markers of three labels (one on several samples, one marker off the domain) and a random region"
    import scipy.ndimage as ndi
    rng = np.random.RandomState(seed)
    shape = tuple(int(n) for n in rng.randint(1, 8, size=3))
    if seed % 3 == 0:
        A = ndi.uniform_filter(rng.randint(0, 200, size=shape).astype(np.float64), 3).astype(np.uint8)
    else:
        A = rng.randint(0, 6, size=shape).astype(np.uint8)
    G = (rng.uniform(size=shape) > 0.15).astype(np.uint8) if walls else None
    M = np.zeros(shape, dtype=np.int32)
    for label in (1, 2, 3, 2, 2):
        M[tuple(rng.randint(0, n) for n in shape)] = label
    return A, M, G


def minimax_levels(A, M, region, connectivity):
    """per label, the least over all paths from its marker samples of the highest sample on the path (walls of 255 where the region
    ends): the reconstruction by erosion from that label's samples alone"""
    assert A.dtype == np.uint8 and A.max() < 255
    walled = A if region is None else np.where(region != 0, A, 255).astype(np.uint8)
    out = {}
    for label in np.unique(M[M > 0]):
        marker = np.where((M == label) & (walled < 255), walled, 255).astype(np.uint8)
        out[int(label)] = recon_ref.reconstruct(walled, marker, method="erosion", connectivity=connectivity)[0]
    return out


def attains_minimax(A, M, region, connectivity, labels):
    "every labelled sample's label is among those whose minimax level at the sample is the least"
    levels = minimax_levels(A, M, region, connectivity)
    best = np.minimum.reduce(list(levels.values()))
    own = np.full(A.shape, 255, dtype=np.uint8)
    for label, level in levels.items():
        own[labels == label] = level[labels == label]
    inside = labels > 0
    return bool(np.all(own[inside] == best[inside])), best


@pytest.mark.parametrize("seed", range(24))
def test_heap_and_fixed_point_agree_and_the_labels_hold_together(seed):
    import scipy.ndimage as ndi
    A, M, G = random_case(seed)
    connectivity = 1 + seed % 3
    for direction in W.DIRECTIONS:
        labels, stats, cost = W.watershed(A, M, G, connectivity, direction, return_cost=True)
        by_heap, stats_h, cost_h = W.watershed(A, M, G, connectivity, direction, cost=W.cost_by_heap, return_cost=True)
        assert np.array_equal(cost, cost_h) and np.array_equal(labels, by_heap) and stats == stats_h
        domain = G != 0
        assert np.array_equal(labels > 0, cost != W.TOP) and not labels[~domain].any()
        assert stats["n_labelled"] + stats["n_unreached"] == int(domain.sum()) and stats["n_ignored"] == int(((M > 0) & ~domain).sum())
        seeds = (M > 0) & domain
        assert np.array_equal(labels[seeds], M[seeds])
        # every region is a union of connected pieces, each holding one of its marker samples
        structure = ndi.generate_binary_structure(3, connectivity)
        for label in np.unique(labels[labels > 0]):
            pieces, k = ndi.label(labels == label, structure=structure)
            for piece in range(1, k + 1):
                assert (M[(pieces == piece) & domain] == label).any(), (seed, direction, label)


@pytest.mark.parametrize("seed", range(12))
def test_every_label_attains_the_minimax_level(seed):
    A, M, G = random_case(seed)
    connectivity = 1 + seed % 3
    labels, _, cost = W.watershed(A, M, G, connectivity, return_cost=True)
    ok, best = attains_minimax(A, M, G, connectivity, labels)
    assert ok
    reached = labels > 0
    assert np.array_equal((cost >> np.uint64(32))[reached], best[reached].astype(np.uint64))      # P is the minimax level
    if reached.sum() > int((M > 0).sum()) + 2 and len(np.unique(labels[reached])) > 1:      # the property test can fail: swap two labels
        a, b = np.unique(labels[reached])[:2]
        swapped = np.where(labels == a, b, np.where(labels == b, a, labels))
        levels = minimax_levels(A, M, G, connectivity)
        if any((levels[int(a)][labels == a] != levels[int(b)][labels == a]).tolist()):
            assert not attains_minimax(A, M, G, connectivity, swapped)[0]


def test_falling_equals_rising_on_complemented_keys():
    for seed in range(6):
        A, M, G = random_case(seed)
        for connectivity in CONNECTIVITIES:
            falling = W.watershed(A, M, G, connectivity, "falling")
            rising = W.watershed((255 - A).astype(np.uint8), M, G, connectivity, "rising")
            assert np.array_equal(falling[0], rising[0]) and falling[1] == rising[1]
    F = np.array([0.5, -0.0, 0.0, np.inf, -np.inf, 2.0], dtype=np.float32).reshape(1, 2, 3)      # the complement of a float's key is the key of -f
    M = np.zeros(F.shape, dtype=np.int32)
    M[0, 0, 0], M[0, 1, 2] = 1, 2
    assert np.array_equal(W.watershed(F, M, direction="falling")[0], W.watershed(-F, M)[0])


def test_a_constant_relief_is_the_geodesic_voronoi_split_with_the_index_rule():
    A = np.full((1, 1, 9), 4, dtype=np.uint8)
    M = np.zeros(A.shape, dtype=np.int32)
    M[0, 0, 0], M[0, 0, 8] = 1, 2
    for direction, connectivity in itertools.product(W.DIRECTIONS, CONNECTIVITIES):
        labels, stats, cost = W.watershed(A, M, None, connectivity, direction, return_cost=True)
        # sample 4 is four steps from both markers; its neighbours 3 and 5 both hold (level, 3): the smaller index, 3, gives its label
        assert labels.reshape(-1).tolist() == [1, 1, 1, 1, 1, 2, 2, 2, 2]
        assert (cost.reshape(-1) & np.uint64(0xFFFFFFFF)).tolist() == [0, 1, 2, 3, 4, 3, 2, 1, 0]
    # in a box the index rule favours the marker that comes first in C order on every exact tie
    B = np.full((1, 5, 5), 4, dtype=np.uint8)
    M = np.zeros(B.shape, dtype=np.int32)
    M[0, 0, 0], M[0, 4, 4] = 1, 2
    labels = W.watershed(B, M)[0][0]
    ties = np.add.outer(np.arange(5), np.arange(5)) == 4
    assert (labels[ties] == 1).all() and (labels == 1).sum() == 15 and (labels == 2).sum() == 10


def test_walls_ignored_markers_and_no_markers():
    A = np.zeros((1, 3, 7), dtype=np.float32)
    G = np.ones(A.shape, dtype=np.uint8)
    G[0, :, 3] = 0      # a wall of the region
    M = np.zeros(A.shape, dtype=np.int32)
    M[0, 0, 0] = 1
    labels, stats = W.watershed(A, M, G)
    assert (labels[0, :, :3] == 1).all() and not labels[0, :, 3:].any() and stats == dict(n_labelled=9, n_unreached=9, n_ignored=0, n_markers=1)
    G[0, 1, 3] = 1      # a gap
    assert W.watershed(A, M, G)[1] == dict(n_labelled=19, n_unreached=0, n_ignored=0, n_markers=1)
    N = A.copy()
    N[0, :, 3] = np.nan      # a wall of NaN, in both directions: NaN is tested on the sample
    M[0, 1, 3], M[0, 2, 6] = 7, 2      # a marker on a NaN sample, and one behind the wall
    for direction in W.DIRECTIONS:
        labels, stats = W.watershed(N, M, None, 3, direction)
        assert (labels[0, :, :3] == 1).all() and (labels[0, :, 4:] == 2).all() and not labels[0, :, 3].any()
        assert stats == dict(n_labelled=18, n_unreached=0, n_ignored=1, n_markers=2)
    G = np.ones(A.shape, dtype=np.uint8)
    G[0, 2, 6] = 0      # a marker outside the region
    labels, stats = W.watershed(N, M, G)
    assert stats == dict(n_labelled=9, n_unreached=8, n_ignored=2, n_markers=1) and not labels[0, :, 3:].any()
    labels, stats = W.watershed(N, np.zeros(A.shape, dtype=np.int32) - 3)      # no markers: nothing is labelled, nothing is an error
    assert not labels.any() and stats == dict(n_labelled=0, n_unreached=18, n_ignored=0, n_markers=0)


def test_one_label_on_two_separated_samples():
    A = np.array([0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0], dtype=np.int16).reshape(1, 1, 13)
    M = np.zeros(A.shape, dtype=np.int32)
    M[0, 0, 0], M[0, 0, 12], M[0, 0, 6] = 5, 5, 8
    labels, stats = W.watershed(A, M)
    # the ridge samples 3 and 9 are wet at level 3 from both sides at once: each takes the side with the smaller index
    assert labels.reshape(-1).tolist() == [5, 5, 5, 5, 8, 8, 8, 8, 8, 8, 5, 5, 5] and stats["n_markers"] == 3
    assert W.watershed(A, M, direction="falling")[0].reshape(-1).tolist() == [5, 5, 5, 5, 8, 8, 8, 8, 8, 8, 5, 5, 5]


def test_scipy_watershed_ift_passes_the_minimax_property_where_its_cost_is_the_level():
    """scipy.ndimage.watershed_ift is no equality oracle: its ties differ, and its arc cost is |f(u) - f(v)|, not the level f(v), so on a
    relief of many levels it does not even attain the minimax level everywhere (measured on the reliefs of random_case: 24 samples of 6 x
    2 cases).  The two costs agree where every climb starts from the level of the markers: a relief of two levels, basins at 0 with the
    markers in them and ridges at 9.  There its output has to pass the property test, ties and all; this checks the property test."""
    import scipy.ndimage as ndi
    rng = np.random.RandomState(7)
    shape = (4, 9, 12)
    A = np.where(ndi.uniform_filter(rng.uniform(size=shape), 3) > 0.52, 9, 0).astype(np.uint8)
    low = np.argwhere(A == 0)
    M = np.zeros(shape, dtype=np.int32)
    for label, at in zip((1, 2, 3, 2), low[rng.choice(len(low), 4, replace=False)]):
        M[tuple(at)] = label
    assert (A == 9).sum() > 40 and (A == 0).sum() > 40
    for connectivity in CONNECTIVITIES:
        theirs = ndi.watershed_ift(A, M, structure=ndi.generate_binary_structure(3, connectivity))
        assert attains_minimax(A, M, None, connectivity, theirs)[0]
        ours = W.watershed(A, M, None, connectivity)[0]
        assert attains_minimax(A, M, None, connectivity, ours)[0]


def test_volume_argument_checks():
    from contourist_amd import volume
    A = np.zeros((3, 4, 5), dtype=np.float32)
    M = np.zeros((3, 4, 5), dtype=np.int32)
    for bad in (dict(direction="up"), dict(connectivity=0), dict(connectivity=4), dict(markers=M[:2]), dict(region=M[:, :3]), dict(markers=M.astype(np.float32))):
        kw = dict(markers=M)
        kw.update(bad)
        with pytest.raises(AssertionError):
            volume.watershed(A, **kw)
    with pytest.raises(AssertionError):
        volume.watershed(np.zeros((2, 2, 2, 2), dtype=np.float32), np.zeros((2, 2, 2, 2), dtype=np.int32))
    for bad in (dict(side="middle"), dict(connectivity=5), dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(sampling=(1.0, 2.0))):
        kw = dict(value=0.5, h=1.0)
        kw.update(bad)
        with pytest.raises(AssertionError):
            volume.split_touching(A, **kw)
    with pytest.raises(AssertionError):
        volume.split_touching(np.zeros((2, 2, 2, 2), dtype=np.float32), 0.5, 1.0)
