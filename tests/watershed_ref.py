"""numpy restatement of cx_grid_watershed3d (include/contourist_hip.h, "watershed"): every sample becomes the unsigned key of the rank
filters (rank_ref.key), the falling direction works on the complemented keys, the arrival cost W = (P, d) of every sample is computed
twice -- by a heap in order of cost, and by relaxing W(v) = min over neighbours u of step(W(u), v) until nothing moves -- and the labels
follow by visiting the samples in order of W, each taking the label of its neighbour of least (W, linear index).  Written from the
header, not from the kernels; not imported by product code.

A cost is one uint64, P << 32 | d, so that the lexicographic order of the pairs is the order of the words; TOP (all ones) stands for
"unreached" and for every sample outside the domain."""
import heapq

import numpy as np

import rank_ref as R

DIRECTIONS = ("rising", "falling")
TOP = np.uint64(0xFFFFFFFFFFFFFFFF)
_32 = np.uint64(32)
_1 = np.uint64(1)


def offsets(connectivity):
    "the neighbours of a sample in C order of their linear index: the offsets that differ from it on 1 .. connectivity axes"
    assert connectivity in (1, 2, 3)
    return [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if 0 < abs(a) + abs(b) + abs(c) <= connectivity]


def working_keys(relief, direction="rising", dtype=None):
    "(the keys the comparisons are made on, as uint64; the samples that are NaN).  NaN is tested on the sample, before the complement"
    assert direction in DIRECTIONS
    A = np.ascontiguousarray(relief)
    assert A.ndim == 3
    name = R.type_name(A, dtype)
    K = R.key(A, dtype)
    ones = K.dtype.type(np.iinfo(K.dtype).max)
    nan = (K == ones) if name in R.FLOATS else np.zeros(A.shape, dtype=bool)
    if direction == "falling":
        K = K ^ ones
    return K.astype(np.uint64), nan


def domain_of(nan, region):
    "inside the region and not NaN"
    inside = np.ones(nan.shape, dtype=bool) if region is None else (np.asarray(region) != 0)
    assert inside.shape == nan.shape
    return inside & ~nan


def cost_by_heap(K, seeds, domain, connectivity):
    "W by settling the samples in order of cost (Dijkstra): a path may not pass through a marker sample, so markers are never entered"
    n = K.shape
    W = np.full(n, TOP, dtype=np.uint64)
    done = np.zeros(n, dtype=bool)
    heap = [(int(K[v]) << 32, v) for v in zip(*(int_axis.tolist() for int_axis in np.nonzero(seeds)))]
    heapq.heapify(heap)
    nb = offsets(connectivity)
    while heap:
        w, v = heapq.heappop(heap)
        if done[v]:
            continue
        done[v] = True
        W[v] = np.uint64(w)
        P = w >> 32
        for o in nb:
            u = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
            if 0 <= u[0] < n[0] and 0 <= u[1] < n[1] and 0 <= u[2] < n[2] and domain[u] and not done[u] and not seeds[u]:
                k = int(K[u])
                heapq.heappush(heap, ((k << 32) if k > P else w + 1, u))
    return W


def cost_by_relaxation(K, seeds, domain, connectivity):
    "W as the fixed point of W(v) = min(W(v), step(W(u), v) over the neighbours u), the marker samples held at (key, 0)"
    n = K.shape
    W = np.full(n, TOP, dtype=np.uint64)
    W[seeds] = K[seeds] << _32
    climb = K << _32
    nb = offsets(connectivity)
    free = domain & ~seeds
    while True:
        P = np.full((n[0] + 2, n[1] + 2, n[2] + 2), TOP, dtype=np.uint64)
        P[1:-1, 1:-1, 1:-1] = W
        best = W.copy()
        for a, b, c in nb:
            U = P[1 + a:1 + a + n[0], 1 + b:1 + b + n[1], 1 + c:1 + c + n[2]]
            stepped = np.where(K > (U >> _32), climb, U + _1)
            np.minimum(best, np.where(U == TOP, TOP, stepped), out=best)
        best = np.where(free, best, W)
        if np.array_equal(best, W):
            return W
        W = best


def parents_of(W, seeds, connectivity):
    """the linear index of the neighbour every reached sample that is no marker takes its label from: least W, among equals the smallest
    index; a marker sample its own index; -1 for the rest"""
    n = W.shape
    lin = np.arange(W.size, dtype=np.int64).reshape(n)
    P = np.full((n[0] + 2, n[1] + 2, n[2] + 2), TOP, dtype=np.uint64)
    P[1:-1, 1:-1, 1:-1] = W
    L = np.full((n[0] + 2, n[1] + 2, n[2] + 2), -1, dtype=np.int64)
    L[1:-1, 1:-1, 1:-1] = lin
    best = np.full(n, TOP, dtype=np.uint64)
    parent = np.full(n, -1, dtype=np.int64)
    for a, b, c in offsets(connectivity):      # ascending linear index: only a strictly lower cost replaces
        U = P[1 + a:1 + a + n[0], 1 + b:1 + b + n[1], 1 + c:1 + c + n[2]]
        better = U < best
        best = np.where(better, U, best)
        parent = np.where(better, L[1 + a:1 + a + n[0], 1 + b:1 + b + n[1], 1 + c:1 + c + n[2]], parent)
    reached = (W != TOP) & ~seeds
    assert np.all(best[reached] < W[reached]), "the neighbour a sample takes its label from has a strictly lower cost"
    parent = np.where(reached, parent, -1)
    return np.where(seeds, lin, parent)


def labels_of(W, markers, seeds, connectivity):
    "the labels, by visiting the samples in order of W"
    parent = parents_of(W, seeds, connectivity).reshape(-1)
    Wf = W.reshape(-1)
    labels = np.zeros(W.size, dtype=np.int32)
    labels[seeds.reshape(-1)] = markers.reshape(-1)[seeds.reshape(-1)]
    for v in np.argsort(Wf, kind="stable").tolist():
        if Wf[v] == TOP:
            break
        if parent[v] != v:
            labels[v] = labels[parent[v]]
    return labels.reshape(W.shape)


def watershed(relief, markers, region=None, connectivity=1, direction="rising", dtype=None, cost=cost_by_relaxation, return_cost=False):
    """cx_grid_watershed3d of a 3-D relief -> (int32 labels, the four exact stats).  dtype='bfloat16': the relief holds uint16 bit
    patterns.  cost: cost_by_relaxation or cost_by_heap"""
    K, nan = working_keys(relief, direction, dtype)
    M = np.asarray(markers)
    assert M.shape == K.shape and M.dtype == np.int32
    domain = domain_of(nan, region)
    seeds = (M > 0) & domain
    W = cost(K, seeds, domain, connectivity)
    labels = labels_of(W, M, seeds, connectivity)
    stats = {"n_labelled": int((labels > 0).sum()), "n_unreached": int((domain & (W == TOP)).sum()),
             "n_ignored": int(((M > 0) & ~domain).sum()), "n_markers": int(seeds.sum())}
    assert stats["n_labelled"] == int((W != TOP).sum())
    return (labels, stats, W) if return_cost else (labels, stats)
