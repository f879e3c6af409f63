"""CPU: the numpy restatement of cx_grid_label3d (tests/label_ref.py) against scipy.ndimage: label with generate_binary_structure(3, c)
bit for bit (scipy numbers components by their first sample in C order, which is the contract's numbering), binary_fill_holes, and
sum / find_objects / center_of_mass for the records."""
import numpy as np
import pytest

import label_ref as R

ndimage = pytest.importorskip("scipy.ndimage")

SHAPES = [(2, 2, 2), (5, 4, 3), (9, 70, 131), (37, 33, 259)]
DENSITIES = [0.5, 0.31, 0.14, 0.1, 0.03]


def uniform(shape, seed):
    return np.random.RandomState(seed).uniform(size=shape).astype(np.float32)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_labels_and_records_against_scipy(shape, connectivity):
    A = uniform(shape, 31)
    structure = ndimage.generate_binary_structure(3, connectivity)
    for density in DENSITIES:
        for side, M in (("high", A >= 1.0 - density), ("low", A < density)):
            value = 1.0 - density if side == "high" else density
            want, k_want = ndimage.label(M, structure)
            got, k = R.label(A, value, side, connectivity)
            assert k == k_want and got.dtype == np.int32
            assert np.array_equal(got, want)
            rec = R.records(got, k)
            assert len(rec) == k
            if k == 0:
                continue
            index = np.arange(1, k + 1)
            assert np.array_equal(rec["voxels"], ndimage.sum(M, want, index).astype(np.int64))
            first = ndimage.minimum(np.arange(M.size).reshape(shape), want, index).astype(np.int64)
            assert np.array_equal(rec["first"], first)
            boxes = ndimage.find_objects(want)
            centres = np.asarray(ndimage.center_of_mass(M, want, index))
            for c in range(0, k, max(1, k // 50)):
                assert tuple(slice(int(lo), int(hi) + 1) for lo, hi in zip(rec["lo"][c], rec["hi"][c])) == boxes[c]
                assert np.allclose(rec["sum"][c] / rec["voxels"][c], centres[c], rtol=1e-12, atol=1e-9)
                rim = 0
                for a in range(3):
                    rim |= (1 << (2 * a)) if boxes[c][a].start == 0 else 0
                    rim |= (2 << (2 * a)) if boxes[c][a].stop == shape[a] else 0
                assert int(rec["rim"][c]) == rim


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_fill_holes_against_scipy(connectivity):
    structure = ndimage.generate_binary_structure(3, connectivity)
    for shape in [(5, 4, 3), (9, 70, 131), (37, 33, 259)]:
        A = uniform(shape, 32)
        for density in (0.5, 0.69, 0.9):
            value = 1.0 - density
            want = ndimage.binary_fill_holes(A >= value, structure).astype(np.uint8)
            assert np.array_equal(R.fill_holes(A, value, connectivity), want)
    # a box with a cavity and a box in the cavity: the cavity is filled, the inner box stays
    B = np.zeros((12, 12, 12), dtype=np.uint8)
    B[1:11, 1:11, 1:11] = 1
    B[3:9, 3:9, 3:9] = 0
    B[5:7, 5:7, 5:7] = 1
    want = ndimage.binary_fill_holes(B, structure).astype(np.uint8)
    got = R.fill_holes(B, 0.5, connectivity)
    assert np.array_equal(got, want) and got[4, 4, 4] == 1 and got[0, 0, 0] == 0


def test_two_dimensions_and_the_other_functions():
    A = uniform((40, 70), 33)
    for connectivity in (1, 2):
        structure = ndimage.generate_binary_structure(2, connectivity)
        want, k_want = ndimage.label(A >= 0.5, structure)
        got, k = R.label(A, 0.5, "high", connectivity)
        assert k == k_want and np.array_equal(got, want)
        assert np.array_equal(R.fill_holes(A, 0.4, connectivity), ndimage.binary_fill_holes(A >= 0.4, structure).astype(np.uint8))
        sizes = ndimage.sum(A >= 0.5, want, np.arange(1, k + 1))
        assert np.array_equal(R.remove_small(A, 0.5, 4, connectivity), (np.concatenate([[0], sizes])[want] >= 4).astype(np.uint8))
        touching = np.unique(np.concatenate([want[0], want[-1], want[:, 0], want[:, -1]]))
        cleared = (A >= 0.5) & ~np.isin(want, touching[touching > 0])
        assert np.array_equal(R.clear_border(A, 0.5, connectivity), cleared.astype(np.uint8))
        biggest = int(np.argmax(sizes)) + 1      # (argmax: the first of equals, the smaller label)
        assert np.array_equal(R.keep_components(A, 0.5, "high", connectivity, largest=1), (want == biggest).astype(np.uint8))
