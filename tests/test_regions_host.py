"""CPU: the numpy restatement of the regions calls (tests/regions_ref.py) against scipy.ndimage and against hand-made cases, and a proof
that the inputs the GPU tests use (tests/test_gpu_regions.py) reach every path of the kernels."""
import numpy as np
import pytest

import regions_ref as R


def _integer_case():
    rng = np.random.RandomState(5)
    L = R.pattern((9, 11, 70), "gaps")
    # every value once: scipy's positions of tied extremes follow its sort, not the C order (ties are tested by hand below)
    V = (rng.permutation(L.size) - 3000).astype(np.int32).reshape(L.shape)
    return L, V


def test_boxes_sums_extremes_and_centres_equal_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    L, V = _integer_case()
    rec = R.regions(L, V)
    k = int(L.max())
    index = np.arange(1, k + 1)
    boxes = ndi.find_objects(L)
    assert len(boxes) == k
    for c, box in enumerate(boxes):
        if box is None:
            assert rec["voxels"][c] == 0 and rec["first"][c] == -1 and tuple(rec["lo"][c]) == (0, 0, 0) and tuple(rec["hi"][c]) == (-1, -1, -1)
            assert rec["min_at"][c] == rec["max_at"][c] == -1 and rec["isum"][c] == 0 and rec["vsum"][c] == 0
            continue
        assert tuple(rec["lo"][c]) == tuple(s.start for s in box) and tuple(rec["hi"][c]) == tuple(s.stop - 1 for s in box)
    present = rec["voxels"] > 0
    assert present.sum() == 9 and not present.all()      # the multiples of 7 only
    assert np.array_equal(rec["voxels"], ndi.sum(np.ones_like(L), L, index).astype(np.int64))
    assert np.array_equal(rec["isum"], ndi.sum(V.astype(np.int64), L, index).astype(np.int64))
    assert np.array_equal(rec["vsum"], rec["isum"].astype(np.float64))
    ids = index[present]
    assert np.array_equal(rec["vmin"][present], ndi.minimum(V, L, ids)) and np.array_equal(rec["vmax"][present], ndi.maximum(V, L, ids))
    lows = [int(np.ravel_multi_index(p, L.shape)) for p in ndi.minimum_position(V, L, ids)]
    highs = [int(np.ravel_multi_index(p, L.shape)) for p in ndi.maximum_position(V, L, ids)]
    assert list(rec["min_at"][present]) == lows and list(rec["max_at"][present]) == highs
    centres = np.asarray(ndi.center_of_mass(np.ones_like(L), L, ids))
    assert np.allclose(rec["sum"][present] / rec["voxels"][present][:, None], centres, rtol=0, atol=1e-12)
    for c in np.flatnonzero(present):
        assert rec["first"][c] == np.flatnonzero(L.reshape(-1) == c + 1)[0]


def test_rim_bits_and_negative_labels():
    L = np.zeros((3, 4, 5), dtype=np.int32)
    L[0, 1, 1] = 1
    L[1, 1:3, 1:4] = 2
    L[2, 3, 4] = 3
    L[1, 0, 0] = -9
    rec = R.regions(L)
    assert list(rec["rim"]) == [1, 0, 2 | 8 | 32] and list(rec["voxels"]) == [1, 6, 1]
    assert len(R.regions(np.full((2, 2, 2), -1))) == 0


def test_float_order_ties_and_nan():
    L = np.ones((1, 1, 8), dtype=np.int32)
    L[0, 0, 7] = 2
    V = np.array([0.0, -0.0, np.nan, 0.0, -0.0, np.inf, np.inf, np.nan], dtype=np.float32).reshape(1, 1, 8)
    rec, abs_sum = R.regions(L, V, with_abs=True)
    assert rec["min_at"][0] == 1 and np.signbit(rec["vmin"][0]) and rec["vmin"][0] == 0      # -0.0 < +0.0, the first -0.0
    assert rec["max_at"][0] == 5 and rec["vmax"][0] == np.inf and rec["n_nan"][0] == 1 and rec["isum"][0] == 0
    assert rec["n_nan"][1] == 1 and rec["min_at"][1] == rec["max_at"][1] == -1 and rec["vmin"][1] == rec["vmax"][1] == rec["vsum"][1] == 0
    bits = (np.array([1.5, -2.0], dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16).reshape(1, 1, 2)
    rec = R.regions(np.ones((1, 1, 2), dtype=np.int32), bits, "bfloat16")
    assert rec["vmin"][0] == -2.0 and rec["vmax"][0] == 1.5 and rec["vsum"][0] == -0.5


def test_integer_ties_go_to_the_smallest_index():
    L = np.array([[[1, 2, 1, 1, 2, 1]]], dtype=np.int32)
    V = np.array([[[7, -3, -5, 7, -3, -5]]], dtype=np.int8)
    rec = R.regions(L, V)
    assert list(rec["min_at"]) == [2, 1] and list(rec["max_at"]) == [0, 1] and list(rec["vmin"]) == [-5, -3] and list(rec["vmax"]) == [7, -3]
    assert list(rec["isum"]) == [4, -6] and list(rec["vsum"]) == [4.0, -6.0]


def test_known_contacts():
    # two boxes that share a face of 3 x 4 samples across axis 2
    L = np.zeros((5, 6, 8), dtype=np.int32)
    L[1:4, 1:5, 1:4] = 1
    L[1:4, 1:5, 4:7] = 2
    got = {(int(r["a"]), int(r["b"])): tuple(int(x) for x in r["faces"]) for r in R.contacts(L)}
    assert got[(1, 2)] == (0, 0, 12)
    assert got[(0, 1)] == (2 * 4 * 3, 2 * 3 * 3, 3 * 4) and got[(0, 2)] == got[(0, 1)]
    assert sorted(got) == [(0, 1), (0, 2), (1, 2)]
    # a label wrapped around another: 2 touches only 1, on all six faces
    L = np.ones((5, 5, 5), dtype=np.int32)
    L[2, 2, 2] = 2
    c = R.contacts(L)
    assert len(c) == 1 and (c["a"][0], c["b"][0]) == (1, 2) and tuple(c["faces"][0]) == (2, 2, 2)
    # labels that meet only along an edge are no contact
    L = np.zeros((2, 2, 2), dtype=np.int32)
    L[0, 0, :] = 1
    L[1, 1, :] = 2
    assert [(int(r["a"]), int(r["b"])) for r in R.contacts(L)] == [(0, 1), (0, 2)]
    # the last sample of a row and the first of the next are no neighbours
    L = np.array([[[1, 1, 1], [2, 2, 2]]], dtype=np.int32)
    c = R.contacts(L)
    assert len(c) == 1 and tuple(c["faces"][0]) == (0, 3, 0)


def test_select_map_and_the_two_selects_agree():
    L = R.pattern((5, 4, 3), "negative")
    keep = np.array([0, 1, 0, 1], dtype=np.uint8)      # shorter than K + 1
    for box, pad in ((None, 0), (None, 2), (((0, 0, 0), (0, 0, 0)), 8), (((4, 3, 2), (4, 3, 2)), 1), (((1, 1, 0), (3, 2, 2)), 3)):
        slow, fast = R.select(L, keep, box, pad), R.select_fast(L, keep, box, pad)
        assert slow[0].tobytes() == fast[0].tobytes() and slow[1:] == fast[1:] and slow[0].shape == fast[0].shape
    mask, origin, ones = R.select(L, keep, None, 1)
    assert origin == (-1, -1, -1) and mask.shape == (7, 6, 5) and ones == int(np.isin(L, (1, 3)).sum())
    assert mask[0].sum() == 0 and mask[:, :, -1].sum() == 0
    table = np.array([5, 2, 2], dtype=np.int32)
    out = R.relabel(L, table)
    assert np.all(out[L <= 0] == 5) and np.all(out[(L == 1) | (L == 2)] == 2) and np.all(out[L > 2] == 0)


def test_the_gpu_inputs_reach_every_path():
    "absent labels, adjacent distinct labels, a region above half the volume, tiles beyond the fallback threshold, ties, overflowing tables"
    gaps = R.pattern(R.STRADDLE, "gaps")
    rec = R.regions(gaps)
    assert (rec["voxels"] == 0).sum() == len(rec) - 9
    one = R.pattern(R.STRADDLE, "one")
    assert R.regions(one)["voxels"][2] == one.size                       # a region larger than half the volume: all of it
    v5 = R.pattern(R.STRADDLE, "voronoi5")
    assert v5.min() == 1 and np.any(v5[:, :, 1:] != v5[:, :, :-1])      # distinct labels side by side in a row, no zeros between
    # a tile of 64 columns with more labels than the wave reduces group by group
    noise = R.pattern(R.STRADDLE, "noise")
    assert len(np.unique(noise[0, 0, :64][noise[0, 0, :64] > 0])) > R.GROUPS_MAX
    v200 = R.pattern(R.STRADDLE, "voronoi200")
    tiles = [len(np.unique(v200[i, j, t:t + 64])) for i in (0, 18, 36) for j in (0, 16, 32) for t in (0, 64, 128, 192)]
    assert 1 < max(tiles) <= R.GROUPS_MAX + 4      # and tiles with a few labels: the group path, several groups deep
    # ties for the minimum and the maximum inside one region, for an integer and a float type
    for name in ("uint8", "float32"):
        V, _ = R.typed_values(R.STRADDLE, name)
        r = R.regions(v5, V, name)
        v = R.as_float64(V, name)
        assert ((v == r["vmin"][0]) & (v5 == 1)).sum() > 1 and ((v == r["vmax"][0]) & (v5 == 1)).sum() > 1
    # the first contact table of a fresh context (512 pairs) overflows on both patterns
    assert len(R.contacts(v200)) > R.TABLE_MIN_PAIRS
    assert len(R.contacts(noise)) > 40 * R.TABLE_MIN_PAIRS
