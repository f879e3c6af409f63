"""The CPU references of tests/buffer_families.py, each run once at size small (the size at which tests/test_gpu_buffers.py compares the
device with them): no case is trivial, so a kernel that did nothing, or copied its input, could not pass there."""
import numpy as np

import buffer_families as F
import label_ref
import levels_ref


def test_the_fields_differ_and_the_quantised_copies_are_rich():
    for size, shape in F.SHAPES3.items():
        A, B = F._field3(size), F.second_field(size)
        assert A.shape == B.shape == shape and A.dtype == B.dtype == np.float32
        assert np.abs(A - B).max() > 0.5
        for name, value in F.TYPED_VALUES.items():
            Q = F.quantised(size, name)
            assert Q.dtype == np.dtype(name) and Q.shape == shape
            assert len(np.unique(Q)) >= 16
            assert (Q == value).any() and (Q < value).any() and (Q > value).any(), (size, name)


def test_filter_changes_the_samples():
    A, (want,) = F._field3("small"), F.filter_expected()
    assert want.shape == A.shape and want.dtype == np.float32 and (want != A).mean() > 0.9


def test_distance_has_sites_and_others():
    A = F._field3("small")
    dist, mask = F.distance_expected()
    low = int((A.astype(np.float64) < F.DISTANCE_VALUE).sum())
    assert 0 < low < A.size
    assert (dist > 0).any() and (dist < 0).any() and len(np.unique(dist)) > 16      # signed: both sides
    assert 0 < int(mask.sum()) < mask.size and int(mask.sum()) > A.size - low         # the mask reaches beyond the sites


def test_label_has_several_components_at_every_connectivity_used():
    A = F._field3("small")
    for c in F.LABEL_CONNECTIVITIES:
        assert label_ref.label(A, F.LABEL_VALUE, "high", c)[1] >= 2, c
    labels, records, mask = F.label_expected()
    k = len(records)
    keep = F.keep_pattern(k)
    assert k >= 2 and labels.max() == k and keep[1:].any() and not keep[1:].all()
    assert 0 < int(mask.sum()) < mask.size and (records["voxels"] > 0).all()


def test_resample_leaves_the_array_and_changes_the_samples():
    A, U = F._field3("small"), F.quantised("small", "uint8")
    (linear, nearest), outside = F.resample_expected(), F.resample_outside()
    assert all(0 < n < A.size for n in outside)
    assert linear.dtype == np.float32 and nearest.dtype == np.uint8
    assert (linear != A).mean() > 0.5 and (nearest != U).mean() > 0.5
    assert (linear == np.float32(F.RESAMPLE_CVAL)).any() and (nearest == 7).any()


def test_rank_changes_the_samples():
    A, Q = F._field3("small"), F.quantised("small", "int16")
    median, maximum = F.rank_expected()
    assert median.dtype == A.dtype and (median != A).mean() > 0.5
    assert maximum.dtype == Q.dtype and (maximum != Q).mean() > 0.5 and (maximum >= Q).all()


def test_reconstruct_changes_the_mask_and_differs_from_the_marker():
    A, U = F._field3("small"), F.quantised("small", "uint8")
    results, stats = F.recon_expected(), F.recon_expected(stats=True)
    for (n_changed, _), got, mask in zip(stats, results, (A, U, A)):
        assert n_changed > 0 and int((got != mask).sum()) == n_changed
    marker = F.recon_marker("small")
    assert stats[2][1] > 0 and (results[2] != marker).any() and (marker > A).any() and (marker < A).any()      # some samples clamped


def test_pick_ranks_and_values_lie_inside_the_data():
    A = F._field3("small")
    got = F.pick_expected()
    assert len(np.unique(got[0])) == 5 and len(np.unique(got[1])) == 5 and F.pick_samples().size != A.size
    spectrum = dict(zip(levels_ref.KEYS, got[2:]))
    assert (spectrum["n_triangles"] > 0).all() and len(np.unique(spectrum["n_triangles"])) == len(F.PICK_VALUES)


def test_every_step_of_a_chain_does_something():
    for op in F.OPERATIONS:
        calls = F.chain_expected(op)
        assert len(calls) == F.CHAIN_CALLS + (op == "reconstruct")
        S = F._field3("small")
        for n, downloads in enumerate(calls[:F.CHAIN_CALLS]):
            out = downloads[-1]
            assert out.shape == S.shape and len(np.unique(out)) >= 2, (op, n)
            assert out.dtype != S.dtype or (out != S).any(), (op, n)
            S = out
        if op == "label":
            assert all(d[0].max() >= 2 for d in calls)      # K of every call
        if op == "reconstruct":
            assert calls[-1][0].shape == (S.shape[0] - 1,) + S.shape[1:] and (calls[-1][0] != S[:-1]).any()
