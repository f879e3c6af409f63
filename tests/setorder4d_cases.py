"""CPython's iteration order of the small sets of lattice points the 4-D march's 2-3 splits depend on, restated in plain numpy
(no GPU, no oracle): the hash of a 4-tuple of small ints, the probe sequence of an 8-slot set, and a scan of a lattice box for
the pentatope splits in which a set member is still on a used slot after its first slots -- the ones the tetrahedra kernel
cannot order from its probe codes (CX4_PROBE_STEPS = 6 slots: the first and five re-probes) and hands to cx_pent_perm_exact,
and the ones its LAST code field decides.

A case is one hyper-voxel `cell` (absolute lattice coordinates of its corner 0), one pentatope `pent` of the 24 (the project's
enumeration, read from csrc/cx_tables4d.h) and one pair `pair` of its five members (m0 < m1): the 2-set is (member m0, member
m1), the 3-set the other three, each inserted in path order, as the reference builds them (pentatopes.py:246-291)."""
import itertools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_M64 = (1 << 64) - 1
_P1 = np.uint64(11400714785074694791)
_P2 = np.uint64(14029467366897019727)
_P5 = np.uint64(2870177450012600261)
PROBE_FIELDS = 6      # CX4_PROBE_STEPS (cx_march4d.hip): slots of a member's probe sequence the kernel keeps


def pent_corners():
    "CX_PENT_CORNERS_INIT of csrc/cx_tables4d.h: 24 x 5 hypercube corners c = 8 di + 4 dj + 2 dk + dl, in path order"
    text = open(os.path.join(ROOT, "contourist_amd", "csrc", "cx_tables4d.h")).read()
    body = text.split("#define CX_PENT_CORNERS_INIT", 1)[1].split("\n}", 1)[0]
    rows = re.findall(r"\{(\d+),(\d+),(\d+),(\d+),(\d+)\}", body)
    P = np.array(rows, dtype=np.int64)
    assert P.shape == (24, 5)
    return P


def corner_offsets(c):
    c = np.asarray(c, dtype=np.int64)
    return np.stack([(c >> 3) & 1, (c >> 2) & 1, (c >> 1) & 1, c & 1], axis=-1)


def hash4(points):
    "hash((i, j, k, l)) of CPython >= 3.8 as uint64, for an (..., 4) array of ints below 2^61 in magnitude"
    p = np.asarray(points, dtype=np.int64)
    lanes = np.where(p == -1, np.int64(-2), p).astype(np.uint64)          # hash(-1) == -2; two's complement
    acc = np.full(p.shape[:-1], _P5, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for d in range(4):
            acc = acc + lanes[..., d] * _P2
            acc = (acc << np.uint64(31)) | (acc >> np.uint64(33))
            acc = acc * _P1
        acc = acc + (np.uint64(4) ^ (_P5 ^ np.uint64(3527539)))
    return np.where(acc == np.uint64(_M64), np.uint64(1546275796), acc)


def probe_sequence(h, steps):
    "slots i0 = h & 7, i_k = (5 i_(k-1) + 1 + (h >> 5k)) & 7 of an 8-slot set (no linear probes at that size) -> (..., steps)"
    h = np.asarray(h, dtype=np.uint64)
    out = np.empty(h.shape + (steps,), dtype=np.int64)
    i = (h & np.uint64(7)).astype(np.int64)
    out[..., 0] = i
    perturb = h.copy()
    for k in range(1, steps):
        perturb = perturb >> np.uint64(5)
        i = (5 * i + 1 + (perturb & np.uint64(7)).astype(np.int64)) & 7
        out[..., k] = i
    return out


def insert_slots(hashes, steps=24):
    """slots of the members of ONE set inserted in order into a fresh 8-slot set -> (slots (..., m), re-probes (..., m)).
    hashes: (..., m) uint64, m <= 3.  (After 13 steps the shifted hash is used up and the recurrence i -> 5 i + 1 visits all 8 slots:
    24 steps always find a free one.)"""
    hashes = np.asarray(hashes, dtype=np.uint64)
    m = hashes.shape[-1]
    slots = np.empty(hashes.shape, dtype=np.int64)
    tries = np.zeros(hashes.shape, dtype=np.int64)
    for n in range(m):
        seq = probe_sequence(hashes[..., n], steps)
        free = np.ones(seq.shape, dtype=bool)
        for e in range(n):
            free &= seq != slots[..., e:e + 1]
        first = np.argmax(free, axis=-1)
        assert free.any(axis=-1).all()
        slots[..., n] = np.take_along_axis(seq, first[..., None], axis=-1)[..., 0]
        tries[..., n] = first
    return slots, tries


def order_of(slots):
    "iteration order of a set = its members by ascending slot -> tuple of insertion indices"
    return tuple(int(x) for x in np.argsort(np.asarray(slots)))


def split_sets(P, pent, pair):
    "members (indices 0..4 into the pentatope's path) of the 2-set and of the 3-set, each in path order"
    two = [m for m in range(5) if m in pair]
    three = [m for m in range(5) if m not in pair]
    return two, three


# (a, b) and (c, d, e) in iteration order give the tetrahedra (ac, be, ad, bd), (ac, be, ad, ae), (ac, be, bd, bc) (pentatopes.py:255-291):
# with both orders reversed the first is itself and the other two change places -- the same three tetrahedra as in insertion order
SAME_AS_UNORDERED = (((0, 1), (0, 1, 2)), ((1, 0), (2, 1, 0)))


def scan(lo, hi, want=8, identity_most=2, negative_only=False, with_two_set=True):
    """the first `want` exact-path cases (a member needs >= PROBE_FIELDS re-probes) and the first `want` boundary cases (the
    worst member needs exactly PROBE_FIELDS - 1: the last field of its code) among the hyper-voxels with lo <= cell <= hi per axis,
    combination by combination (pentatope, pair), at most one case of a kind per pentatope, the pentatopes taken in turn from the
    four groups of six the tetrahedra kernel instantiates separately (cx_tets_group<0..3>).  In most cases the member that runs out
    of slots is the third of the 3-set (two used slots); the scan goes on until one exact case is found in which it is the second
    member of the 2-set (`exact[-1]`, replacing the last).  Of the exact cases at most `identity_most` may have both sets iterate in insertion order (a kernel that
    ordered nothing would pass those).  negative_only: only hyper-voxels with a negative coordinate."""
    P = pent_corners()
    ax = np.arange(lo, hi + 1, dtype=np.int64)
    cells = np.stack(np.meshgrid(ax, ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 4)
    if negative_only:
        cells = cells[(cells < 0).any(axis=1)]
    H = [hash4(cells + corner_offsets(c)) for c in range(16)]           # per corner of the hyper-voxel
    exact, boundary, n_identity = [], [], 0
    taken = {}
    two_set_case = None if with_two_set else False      # False: not looked for
    for pent in [6 * g + n for n in range(6) for g in range(4)]:
        for pair in itertools.combinations(range(5), 2):
            two, three = split_sets(P, pent, pair)
            s2, t2 = insert_slots(np.stack([H[P[pent][m]] for m in two], axis=-1))
            s3, t3 = insert_slots(np.stack([H[P[pent][m]] for m in three], axis=-1))
            worst = np.maximum(t2.max(axis=-1), t3.max(axis=-1))
            for kind, out, sel in (("exact", exact, np.flatnonzero(worst >= PROBE_FIELDS)),
                                   ("boundary", boundary, np.flatnonzero(worst == PROBE_FIELDS - 1))):
                for x in sel:
                    two_set = kind == "exact" and two_set_case is None and t2[x].max() >= PROBE_FIELDS
                    if (len(out) >= want or taken.get((kind, pent), 0) >= 1) and not two_set:
                        break
                    o2, o3 = order_of(s2[x]), order_of(s3[x])
                    identity = (o2, o3) in SAME_AS_UNORDERED
                    if kind == "exact" and identity:
                        if n_identity >= identity_most or two_set:
                            continue
                        n_identity += 1
                    case = dict(cell=tuple(int(v) for v in cells[x]), pent=pent, pair=pair,
                                    two=[tuple(int(v) for v in cells[x] + corner_offsets(P[pent][m])) for m in two],
                                    three=[tuple(int(v) for v in cells[x] + corner_offsets(P[pent][m])) for m in three],
                                    corners2=[int(P[pent][m]) for m in two],
                                    order2=o2, order3=o3, reprobes=tuple(int(v) for v in t2[x]) + tuple(int(v) for v in t3[x]))
                    if two_set:
                        two_set_case = case
                    else:
                        out.append(case)
                        taken[(kind, pent)] = taken.get((kind, pent), 0) + 1
            if len(exact) >= want and len(boundary) >= want and two_set_case is not None:
                break
        else:
            continue
        break
    if two_set_case:
        exact = exact[:want - 1] + [two_set_case]
    return exact, boundary


_CACHE = {}


def selected(lo, hi, want=8, negative_only=False):
    "scan(), once per process and box (the small negative box holds too few sets to wait for a 2-set case)"
    key = (lo, hi, want, negative_only)
    if key not in _CACHE:
        _CACHE[key] = scan(lo, hi, want, negative_only=negative_only, with_two_set=not negative_only)
    return _CACHE[key]


# the boxes the tests use: origin 0 (the reference's own lattice) and one that starts at -3 (cells with negative coordinates
# and the -1 whose hash is -2; scanned with negative_only)
BOX_POSITIVE = (0, 11)
BOX_NEGATIVE = (-3, 4)
