"""Fields, cases and the device-against-oracle comparison of the seeded selections (cx_seed.hip, cx_seed4.hip), shared by
tests/test_seeds_oracle_host.py, tests/test_gpu_seeded.py, tests/test_gpu_seeded4d.py and tools/fuzz_gpu_seeded.py.

The fields are separated noisy spheres: min_i(|x - c_i| - r_i) + ripple * prod_a sin(0.9 x_a + a), isovalue 0, generated here.
Every comparison is exact: kept triangles / tetrahedra as sets of sorted edge-key tuples, the counts, the vertex mask (3-D) and
groups_kept against oracle/seeds.py."""
import numpy as np

FIELD3 = dict(shape=(40, 38, 41), ripple=0.35, radii=(8.3, 8.6, 7.4, 3.2),
              centres=((11.3, 11.1, 11.2), (28.2, 27.4, 12.1), (12.4, 26.6, 29.3), (30.5, 10.5, 30.5)))
FIELD4 = dict(shape=(14, 15, 14, 8), ripple=0.15, radii=(3.1, 3.3, 1.3),
              centres=((4.2, 4.1, 4.3, 3.4), (9.6, 10.4, 9.5, 3.7), (4.5, 11.0, 4.2, 5.6)))
# far-apart end point pairs (one point deep inside a sphere, the other outside it and beyond a neighbouring sphere: several
# bisection steps), named by the number of surface voxels of the component the restated search reaches from them.  The tests
# assert that number from the oracle before they touch the device.
PAIRS3 = {1306: [(11, 11, 11), (39, 0, 40)], 1416: [(28, 27, 12), (0, 0, 40)], 1036: [(12, 27, 29), (39, 0, 0)],
          194: [(30, 10, 30), (0, 37, 0)]}
PAIRS4 = {1032: [(4, 4, 4, 3), (13, 14, 0, 0)], 1238: [(10, 10, 10, 4), (0, 0, 13, 0)], 102: [(4, 11, 4, 6), (13, 0, 0, 0)]}

_CACHE = {}


def spheres(shape, centres, radii, ripple):
    ax = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    d = np.min([np.sqrt(sum((x - c[a]) ** 2 for a, x in enumerate(ax))) - r for c, r in zip(centres, radii)], axis=0)
    w = np.ones(shape)
    for a, x in enumerate(ax):
        w = w * np.sin(0.9 * x + a)
    return (d + ripple * w).astype(np.float32)


def field3d():
    if "A3" not in _CACHE:
        _CACHE["A3"] = spheres(**FIELD3)
        _CACHE["A3"].setflags(write=False)
    return _CACHE["A3"], 0.0


def field4d():
    if "A4" not in _CACHE:
        _CACHE["A4"] = spheres(**FIELD4)
        _CACHE["A4"].setflags(write=False)
    return _CACHE["A4"], 0.0


def flipped(pair):
    "the pair as (high, low): the selection orders the points itself"
    return [pair[1], pair[0]]


def assert_preconditions(A, value):
    """what makes a field exercise the far unions on a kept group, from the oracle alone: no sample equals the isovalue (the
    reference's border voxels are then the voxels with triangles), at least three components, two of them with more than 1024
    voxels (records of one group in two blocks of CXS_UB / CXS4_UB = 1024 consecutive records).  -> the component sizes"""
    from oracle import seeds
    key = ("groups", id(A), float(value))
    if key not in _CACHE:
        _CACHE[key] = (A, [n for n, _ in seeds.groups(A, value, ())])       # (A held: its id stays its own)
    sizes = _CACHE[key][1]
    assert not np.any(np.asarray(A, dtype=np.float64) == value), "a sample equals the isovalue"
    assert len(sizes) >= 3, sizes
    assert sum(1 for n in sizes if n > 1024) >= 2, sizes
    return sizes


class OracleMesh:
    "the oracle's Level-0 mesh of a field (marched once per field) and the restated selection on it"

    def __init__(self, A, value):
        from oracle import level0, level0_4d
        self.A, self.value, self.dim = A, float(value), A.ndim
        A32 = np.ascontiguousarray(A, dtype=np.float32)
        assert np.array_equal(A32.astype(np.float64), np.asarray(A, dtype=np.float64))     # the march reads fp32: nothing lost
        if self.dim == 3:
            self.O = level0.march3d(A32, value, diag_mode=1)
            self.keys = level0.edge_keys_from_pairs(self.O["pairs"], A.shape)
            self.cells = self.O["tris"]
        else:
            self.O = level0_4d.march4d(A32, value, diag_mode=1)
            self.keys = level0_4d.edge_keys4(self.O["pairs"], A.shape)
            self.cells = self.O["tets"]
        self.rows = [tuple(r) for r in np.sort(self.keys[self.cells], axis=1).tolist()] if len(self.cells) else []

    def select(self, case):
        "-> (mask over the oracle's simplices, kept voxels)"
        from oracle import seeds
        box = case.get("box")
        lo, hi = (None, None) if box is None else box
        how = dict(all_in_range=bool(case.get("all_in_range")), shared_visited=not case.get("parallel"), strict=bool(case.get("strict")))
        how.update(case.get("oracle", {}))
        f = seeds.select if self.dim == 3 else seeds.select4d
        return f(self.A, self.value, case["eps"], self.keys, self.cells, lo, hi, **how)

    def kept_rows(self, mask):
        return set(r for r, m in zip(self.rows, mask) if m)


def oracle_mesh(A, value):
    key = ("mesh", id(A), float(value))
    if key not in _CACHE:
        _CACHE[key] = (A, OracleMesh(A, value))
    return _CACHE[key][1]


def case(eps, box=None, all_in_range=False, parallel=False, strict=False):
    """one selection: end point pairs, in_range box (lo, hi) or None, CX_SEED_ALL_IN_RANGE, the one-thread-per-pair seed kernel
    (and the oracle without the shared visited set), strict: the oracle with the march's strict sign change as border rule"""
    return dict(eps=[[tuple(int(x) for x in a), tuple(int(x) for x in b)] for a, b in eps], box=box, all_in_range=all_in_range,
                parallel=parallel, strict=strict)


class DeviceMesh:
    "one context with a field uploaded and marched (3-D or 4-D), its Level-0 mesh on the host"

    def __init__(self, A, value, ctx=None, native=False):
        from contourist_amd import _ffi
        self.ctx = ctx if ctx is not None else _ffi.Context(0)
        self.dim = A.ndim
        if self.dim == 3:
            (self.ctx.upload_grid_native if native else self.ctx.upload_grid)(A)
            self.counts = self.ctx.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
            _, keys, self.cells = self.ctx.download_level0(self.counts)
        else:
            self.ctx.upload_grid4d(A)
            self.counts = self.ctx.extract4d(value, _ffi.CX_DIAG_CPYTHON310)
            _, keys, self.cells = self.ctx.download_level0_4d(self.counts)
        self.keys = keys.astype(np.int64)
        self.rows = [tuple(r) for r in np.sort(self.keys[self.cells.astype(np.int64)], axis=1).tolist()] if len(self.cells) else []

    def select(self, c):
        "-> (counts of the call, simplex mask, vertex mask or None)"
        if self.dim == 3:
            got = self.ctx.select_seeded(c["eps"], c.get("box"), bool(c.get("all_in_range")), bool(c.get("parallel")))
            tk, vk = self.ctx.seeded_masks(self.counts)
            return dict(got, kept=got["triangles_kept"]), tk, vk
        got = self.ctx.select_seeded4d(c["eps"], c.get("box"), bool(c.get("all_in_range")), bool(c.get("parallel")))
        return dict(got, kept=got["tetrahedra_kept"]), self.ctx.seeded4d_mask(self.counts).astype(bool), None

    def kept_rows(self, mask):
        return set(r for r, m in zip(self.rows, mask) if m)

    def close(self):
        self.ctx.close()


def run_case(D, M, c):
    """the selection `c` on the device mesh D and on the oracle mesh M -> dict(mismatches: list of str (empty: equal), got: the
    device's counts, want: the oracle's mask, surf: the oracle's kept voxels, groups: the oracle's (size, kept) per in-box group)"""
    from oracle import seeds
    want, surf = M.select(c)
    got, mask, vmask = D.select(c)
    bad = []
    dev, ora = D.kept_rows(mask), M.kept_rows(want)
    if dev != ora:
        bad.append("kept simplices differ: %d on the device only, %d in the oracle only" % (len(dev - ora), len(ora - dev)))
    if len(dev) != int(mask.sum()):
        bad.append("a kept simplex twice")
    if got["kept"] != int(want.sum()) or got["kept"] != int(mask.sum()):
        bad.append("count %d, mask %d, oracle %d" % (got["kept"], int(mask.sum()), int(want.sum())))
    if vmask is not None:
        used = np.zeros(len(vmask), dtype=bool)
        used[np.asarray(D.cells)[mask].ravel()] = True
        if not np.array_equal(used, vmask):
            bad.append("vertex mask is not `used by a kept triangle`: %d differ" % int((used != vmask).sum()))
    box = c.get("box")
    lo, hi = (None, None) if box is None else box
    groups = seeds.groups(M.A, M.value, surf, lo, hi, bool(c.get("strict")))
    if any(k not in (0, n) for n, k in groups):
        bad.append("the oracle keeps a group in part: %r" % (groups,))
    if got["groups_kept"] != sum(1 for n, k in groups if k):
        bad.append("groups_kept %d, oracle %d" % (got["groups_kept"], sum(1 for n, k in groups if k)))
    mode = D.ctx.seeded_mode()
    if mode != ("parallel" if c.get("parallel") or len(c["eps"]) > (65536 if D.dim == 3 else 16384) else "sequential"):
        bad.append("seed kernel: " + mode)
    return dict(mismatches=bad, got=got, want=want, surf=surf, groups=groups, mask=mask)


def reference_crossing_segments(S, gd, value):
    """every crossing lattice segment of the reference's exhaustive search (grid_field.py:64-84), in its order: from every lattice
    point 0 <= p < gd (index order, last axis fastest) to its 2^d - 1 forward neighbours (first axis fastest), strict sign change.
    S: samples at the lattice points 0 .. gd inclusive"""
    d = len(gd)
    out = []
    for p in np.ndindex(*[int(n) for n in gd]):
        for index in range(1, 2 ** d):
            q = tuple(p[a] + ((index >> a) & 1) for a in range(d))
            if (S[p] - value) * (S[q] - value) < 0:
                out.append((p, q))
    return out


# ---- random cases (tools/fuzz_gpu_seeded.py) ---------------------------------------------------------------------------------

def random_field(rng, dim=3):
    "three to five noisy spheres in a random grid; isovalue 0"
    shape = tuple(int(x) for x in (rng.randint(22, 40, size=3) if dim == 3 else rng.randint(9, 15, size=4)))
    n = int(rng.randint(3, 6))
    centres = [tuple(rng.uniform(0.15 * s, 0.85 * s) for s in shape) for _ in range(n)]
    radii = [float(rng.uniform(0.08, 0.26) * min(shape[:3])) for _ in range(n)]
    return spheres(shape, centres, radii, float(rng.uniform(0.05, 0.4))), 0.0


def random_case(rng, A, value):
    "far-apart end point pairs (a random low and a random high sample each), a random box, now and then ALL_IN_RANGE / parallel"
    low, high = np.argwhere(A < value), np.argwhere(A > value)
    eps = []
    for _ in range(int(rng.randint(1, 5))):
        pair = [low[rng.randint(len(low))], high[rng.randint(len(high))]]
        eps.append(pair if rng.rand() < 0.5 else pair[::-1])
    if rng.rand() < 0.3:
        eps.append(eps[0])
    box = None
    if rng.rand() < 0.75:
        n = np.array(A.shape)
        lo = np.array([rng.randint(-2, max(s // 2, 1)) for s in n])
        hi = np.array([rng.randint(s // 2, s + 3) for s in n])
        if rng.rand() < 0.1:
            a = int(rng.randint(A.ndim))
            hi[a] = lo[a]                                   # empty: only the seed voxels are kept
        box = (tuple(int(x) for x in lo), tuple(int(x) for x in hi))
    return case(eps, box, all_in_range=rng.rand() < 0.2, parallel=rng.rand() < 0.3)


# ---- the documented deviation: voxels that only touch the isovalue do not bridge groups ----------------------------------------

def bridge_field(dim=3):
    """two low cubes in a high field, three samples apart along axis 0, and between them ONE sample equal to the isovalue 0 among
    higher ones.  The reference's border_voxel (min <= value <= max) makes the 2^dim voxels around that sample border voxels: they
    touch the last voxels of both cubes and bridge the two groups.  The march sees no sign change there (a sample equal to the
    isovalue is high).  -> (A, isovalue, end point pair inside the first cube's surface)"""
    shape = (17, 10, 10) if dim == 3 else (17, 9, 9, 6)
    A = np.ones(shape, dtype=np.float32)
    mid = tuple(slice(3, 7) for _ in range(dim - 1)) if dim == 3 else (slice(3, 7), slice(3, 7), slice(2, 5))
    A[(slice(3, 7),) + mid] = -1.0
    A[(slice(10, 14),) + mid] = -1.0
    touch = (8, 5, 5) if dim == 3 else (8, 5, 5, 3)
    A[touch] = 0.0
    a = (4, 5, 5) if dim == 3 else (4, 5, 5, 3)
    return A, 0.0, [a, (0,) + a[1:]]


# adjacent pairs whose high points' own voxels are not border voxels and share candidate neighbours: with the reference's shared
# visited set the later pair moves on to another voxel, without it (the parallel seed kernels) it takes the same one
COLLIDING3 = [[(7, 29, 26), (6, 29, 26)], [(7, 29, 32), (6, 29, 32)], [(7, 30, 27), (6, 30, 27)]]
COLLIDING4 = [[(2, 3, 3, 2), (1, 3, 3, 2)], [(2, 4, 4, 3), (1, 4, 4, 3)]]
