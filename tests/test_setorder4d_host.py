"""CPU: tests/setorder4d_cases.py against this interpreter -- the tuple hash, and the iteration order of real sets built from the
selected pentatope splits.  This is the ground truth the reference's 2-3 splits rest on (pentatopes.py:246-291 iterates sets of
lattice points), independent of the oracle; the GPU test of the exact set order (test_gpu_march4d_paths.py) takes its cases from
the same selection."""
import sys

import numpy as np
import pytest

import setorder4d_cases as S

pytestmark = pytest.mark.skipif(sys.implementation.name != "cpython" or sys.version_info < (3, 8),
                                reason="the tuple hash restated here is CPython's since 3.8")


def test_hash_of_four_tuples_equals_the_interpreters():
    rng = np.random.RandomState(7)
    T = np.concatenate([rng.randint(-3, 40, size=(3000, 4)), rng.randint(-3, 1 << 31, size=(1000, 4)),
                        np.array([[-1, -1, -1, -1], [0, 0, 0, -1], [-1, 0, 0, 0], [-2, -1, -3, 5], [0, 0, 0, 0]])]).astype(np.int64)
    h = S.hash4(T)
    for row, got in zip(T.tolist(), h.tolist()):
        assert got == hash(tuple(row)) & (2 ** 64 - 1), row


def _cases():
    ep, bp = S.selected(*S.BOX_POSITIVE)
    en, bn = S.selected(*S.BOX_NEGATIVE, want=2, negative_only=True)
    return ep, bp, en, bn


def test_selection_is_not_empty_and_is_what_it_says():
    ep, bp, en, bn = _cases()
    assert len(ep) >= 8 and len(bp) >= 8
    assert len(en) >= 1 and len(bn) >= 1
    for c in ep + en:
        assert max(c["reprobes"]) >= S.PROBE_FIELDS
    for c in bp + bn:
        assert max(c["reprobes"]) == S.PROBE_FIELDS - 1
    for c in en + bn:
        assert min(c["cell"]) < 0
    # both sets run out of code somewhere, several pentatope groups, and orders a kernel that ordered nothing would get wrong
    assert any(max(c["reprobes"][:2]) >= S.PROBE_FIELDS for c in ep) and any(max(c["reprobes"][2:]) >= S.PROBE_FIELDS for c in ep)
    assert len(set(c["pent"] // 6 for c in ep)) == 4 and len(set(c["pent"] // 6 for c in bp)) == 4
    assert sum((c["order2"], c["order3"]) not in S.SAME_AS_UNORDERED for c in ep) >= 6
    P = S.pent_corners()
    for c in ep + bp + en + bn:      # the sets are the pentatope's five points, in path order (each step raises one coordinate)
        pts = [tuple(int(v) for v in np.array(c["cell"]) + S.corner_offsets(P[c["pent"]][m])) for m in range(5)]
        assert sorted(c["two"] + c["three"]) == sorted(pts) and len(set(pts)) == 5
        assert [p for p in pts if p in c["two"]] == c["two"] and [p for p in pts if p in c["three"]] == c["three"]
        assert all(sum(b) - sum(a) == 1 for a, b in zip(pts, pts[1:]))


def test_order_of_real_sets():
    "a real set, its members inserted in path order, iterates in the order the helper computed"
    for c in sum(_cases(), []):
        for members, order in ((c["two"], c["order2"]), (c["three"], c["order3"])):
            s = set()
            for p in members:
                s.add(p)
            assert list(s) == [members[n] for n in order], (c, members)


def test_probe_sequence_against_a_scalar_restatement():
    "setobject.c's loop for a table of 8 slots, one hash at a time"
    rng = np.random.RandomState(3)
    hs = [int(x) for x in rng.randint(0, 1 << 62, size=200)] + [2 ** 64 - 2, 0, 7]
    seq = S.probe_sequence(np.array(hs, dtype=np.uint64), 16)
    for h, row in zip(hs, seq.tolist()):
        i, perturb, want = h & 7, h, []
        for _ in range(16):
            want.append(i)
            perturb >>= 5
            i = (i * 5 + 1 + perturb) & 7
        assert row == want
