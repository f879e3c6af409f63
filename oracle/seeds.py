"""TEST INFRASTRUCTURE (oracle) -- seeded voxel selection of the 3-D and the 4-D march, restated from the reference
(the 4-D march reuses the same methods with the 80 offsets of pentatopes.py:32-39).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this package.

Reference (contourist/tetrahedral.py):
  OFFSETS               :41-47    the 26 neighbour offsets in (i, j, k) lexicographic order
  border_voxel          :383-394  not np.allclose(value, corners) and min <= value <= max
  find_initial_voxels   :396-441  bisection of each end point pair, the point's own voxel or its first border
                                  neighbour, one shared `visited` set
  expand_voxels         :443-463  breadth-first growth over in-range border voxels
  in_range              :465-469  0 <= voxel < corner
The reference evaluates f outside the array for voxels on its rim; a dense array cannot: such voxels are not
border voxels here (the same rule as the device code)."""
import itertools

import numpy as np

OFFSETS = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
BOX = list(itertools.product((0, 1), repeat=3))
_OFFS = {3: OFFSETS, 4: [o for o in itertools.product((-1, 0, 1), repeat=4) if any(o)]}
_BOX = {3: BOX, 4: list(itertools.product((0, 1), repeat=4))}


def border_voxel(A, value, p, strict=False):
    """the reference's border_voxel (:383-394) at voxel p.  strict=True: a strict sign change among the corners instead, by the
    march's rule that a sample equal to the isovalue is high (the voxels that emit triangles / tetrahedra)"""
    p = tuple(int(x) for x in p)
    dim = A.ndim
    if any(x < 0 for x in p) or any(p[a] + 1 >= A.shape[a] for a in range(dim)):
        return False
    vals = np.array([float(A[tuple(p[a] + b[a] for a in range(dim))]) for b in _BOX[dim]], dtype=np.float64)
    if strict:
        high = vals >= value
        return bool(high.any() and not high.all())
    if np.allclose(value, vals):
        return False
    return vals.min() <= value and vals.max() >= value


def border_mask(A, value, strict=False):
    "border_voxel of every voxel at once: boolean array of shape A.shape - 1 (same rules, same arithmetic in float64)"
    A64 = np.asarray(A, dtype=np.float64)
    dim = A64.ndim
    corners = [A64[tuple(slice(b[a], A64.shape[a] - 1 + b[a]) for a in range(dim))] for b in _BOX[dim]]
    if strict:
        high = [c >= value for c in corners]
        return np.logical_or.reduce(high) & ~np.logical_and.reduce(high)
    close = np.logical_and.reduce([np.abs(value - c) <= 1e-8 + 1e-5 * np.abs(c) for c in corners])   # np.allclose(value, corners)
    return ~close & (np.minimum.reduce(corners) <= value) & (np.maximum.reduce(corners) >= value)


def _border_test(A, value, strict, vectorised):
    "p -> bool: the scalar border_voxel, or a look-up in border_mask (the same answers, tests/test_seeds_oracle_host.py)"
    if not vectorised:
        return lambda p: border_voxel(A, value, p, strict)
    mask = border_mask(A, value, strict)
    shape = mask.shape

    def test(p):
        for x, n in zip(p, shape):
            if x < 0 or x >= n:
                return False
        return bool(mask[tuple(p)])
    return test


def _bisect(A, value, low_point, high_point):
    low_point, high_point = low_point.copy(), high_point.copy()
    low_value, high_value = float(A[tuple(low_point)]), float(A[tuple(high_point)])
    if low_value > value or high_value < value:
        low_point, low_value, high_point, high_value = high_point, high_value, low_point, low_value
    assert low_value <= value and high_value >= value, "Bad end points"
    while np.any(np.abs(low_point - high_point) > 1):
        mid = (low_point + high_point) // 2
        if float(A[tuple(mid)]) < value:
            low_point = mid
        else:
            high_point = mid
    return low_point, high_point


def initial_voxels(A, value, end_points, shared_visited=True, strict=False, vectorised=True):
    """find_initial_voxels (:396-441).  shared_visited=False: what the one-thread-per-pair seed kernels compute (cxs_k_seeds_parallel,
    cxs4_k_seeds_parallel): every end point on its own yields its voxel if that is a border voxel, else its first border neighbour
    in OFFSETS order -- no `visited` set.  Pairs are independent then, so the pair list is deduplicated first (exact)."""
    dim = A.ndim
    is_border = _border_test(A, value, strict, vectorised)
    pairs = np.asarray(end_points, dtype=np.int64).reshape(-1, 2, dim)
    new = set()
    if not shared_visited:
        for pair in np.unique(pairs.reshape(-1, 2 * dim), axis=0).reshape(-1, 2, dim):
            for point in _bisect(A, value, pair[0], pair[1]):
                t = tuple(int(x) for x in point)
                if is_border(t):
                    new.add(t)
                    continue
                for o in _OFFS[dim]:
                    q = tuple(t[a] + o[a] for a in range(dim))
                    if is_border(q):
                        new.add(q)
                        break
        return new
    visited = set()
    for (low_point, high_point) in pairs:
        for point in _bisect(A, value, low_point, high_point):
            t = tuple(int(x) for x in point)
            if t in visited:
                continue
            visited.add(t)
            if is_border(t):
                new.add(t)
                continue
            for o in _OFFS[dim]:
                q = tuple(t[a] + o[a] for a in range(dim))
                if q in visited:
                    continue
                visited.add(q)
                if is_border(q):
                    new.add(q)
                    break
    return new


def _box(A, lo, hi):
    "the in_range box clamped to the array: lo <= voxel < hi"
    dim = A.ndim
    corner = np.array(A.shape) - 1 if hi is None else np.minimum(np.array(hi), np.array(A.shape) - 1)
    lo = np.zeros(dim, dtype=int) if lo is None else np.maximum(np.array(lo), 0)
    return [int(x) for x in lo], [int(x) for x in corner]


def expand(A, value, seeds, lo=None, hi=None, strict=False, vectorised=True):
    """lo <= voxel < hi is the reference's in_range box (default: the whole array).  The seeds themselves are not range-checked
    (as in the reference): one outside the box is kept and grows one step into it."""
    lo, corner = _box(A, lo, hi)
    dim = A.ndim
    is_border = _border_test(A, value, strict, vectorised)
    surface, visited, horizon = set(), set(seeds), set(seeds)
    while horizon:
        nxt = set()
        for v in horizon:
            surface.add(v)
            for o in _OFFS[dim]:
                q = tuple(v[a] + o[a] for a in range(dim))
                if q in visited or any(q[a] < lo[a] or q[a] >= corner[a] for a in range(dim)):
                    continue
                visited.add(q)
                if is_border(q):
                    nxt.add(q)
        horizon = nxt
    return surface


def in_box_surface(A, value, lo=None, hi=None, strict=False):
    "every border voxel inside the in_range box, as a set of tuples"
    lo, corner = _box(A, lo, hi)
    mask = border_mask(A, value, strict)
    inside = np.zeros_like(mask)
    if all(l < c for l, c in zip(lo, corner)):
        inside[tuple(slice(l, c) for l, c in zip(lo, corner))] = True
    return set(tuple(int(x) for x in p) for p in np.argwhere(mask & inside))


def reached(A, value, end_points, lo=None, hi=None, all_in_range=False, shared_visited=True, strict=False, vectorised=True):
    """the voxels a seeded selection keeps.  all_in_range (CX_SEED_ALL_IN_RANGE): every surface voxel inside the box, whatever
    its group, and the initial voxels (those outside the box are all the end points add)."""
    initial = initial_voxels(A, value, end_points, shared_visited, strict, vectorised)
    if all_in_range:
        return in_box_surface(A, value, lo, hi, strict) | initial
    return expand(A, value, initial, lo, hi, strict, vectorised)


def groups(A, value, kept, lo=None, hi=None, strict=False):
    """the 26-/80-connected groups among the surface voxels INSIDE the box (connected inside the box), largest first:
    list of (number of voxels, how many of them `kept` contains).  What groups_kept of the device counts: the groups with
    a kept voxel (a group is kept whole or not at all); a seed voxel outside the box is no group."""
    dim = A.ndim
    todo = in_box_surface(A, value, lo, hi, strict)
    kept = set(kept)
    out = []
    while todo:
        start = todo.pop()
        comp, horizon = {start}, [start]
        while horizon:
            v = horizon.pop()
            for o in _OFFS[dim]:
                q = tuple(v[a] + o[a] for a in range(dim))
                if q in todo:
                    todo.remove(q)
                    comp.add(q)
                    horizon.append(q)
        out.append((len(comp), len(comp & kept), min(comp)))
    out.sort(key=lambda g: (-g[0], g[2]))
    return [(n, k) for n, k, _ in out]


def groups_kept(A, value, kept, lo=None, hi=None, strict=False):
    return sum(1 for n, k in groups(A, value, kept, lo, hi, strict) if k)


def triangle_voxels(keys, tris, shape):
    """lower corner of the voxel that emitted each Level-0 triangle: the componentwise minimum over the lattice
    end points of its three edges (every Kuhn tetrahedron contains corner 0 of its voxel)"""
    keys = np.asarray(keys, dtype=np.int64)
    lin, d = keys >> 3, keys & 7
    q = np.stack([lin // (shape[1] * shape[2]), (lin // shape[2]) % shape[1], lin % shape[2]], axis=1)
    return q[np.asarray(tris)].min(axis=1)


def _mask_of(vox, surf, shape):
    inside = np.zeros(tuple(shape), dtype=bool)
    if surf:
        inside[tuple(np.array(sorted(surf), dtype=np.int64).T)] = True
    vox = np.asarray(vox, dtype=np.int64).reshape(-1, len(shape))
    return inside[tuple(vox.T)] if len(vox) else np.zeros(0, dtype=bool)


def select(A, value, end_points, keys, tris, lo=None, hi=None, **how):
    """mask over the Level-0 triangles: emitted by a voxel the reference's seeded search reaches, and those voxels;
    how: all_in_range, shared_visited, strict, vectorised of reached()"""
    surf = reached(A, value, end_points, lo, hi, **how)
    return _mask_of(triangle_voxels(keys, tris, A.shape), surf, A.shape), surf


def tetrahedron_voxels(keys, tets, shape):
    """lower corner of the hyper-voxel that emitted each Level-0 tetrahedron of the 4-D march: the componentwise
    minimum over the owners of its four edges (every tetrahedron touches all five corners of its pentatope, and every
    pentatope contains corner 0 of its hypercube)"""
    keys = np.asarray(keys, dtype=np.int64)
    lin = keys >> 4
    s3, s2, s1 = shape[3], shape[2] * shape[3], shape[1] * shape[2] * shape[3]
    q = np.stack([lin // s1, (lin // s2) % shape[1], (lin // s3) % shape[2], lin % shape[3]], axis=1)
    return q[np.asarray(tets)].min(axis=1)


def select4d(A, value, end_points, keys, tets, lo=None, hi=None, **how):
    "mask over the Level-0 tetrahedra: emitted by a hyper-voxel the reference's seeded search reaches (how: as select)"
    surf = reached(A, value, end_points, lo, hi, **how)
    return _mask_of(tetrahedron_voxels(keys, tets, A.shape), surf, A.shape), surf
