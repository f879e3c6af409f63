"""Hand-made meshes with known topology for tests/test_topology_host.py and tests/test_gpu_topology.py: (points, triangles).
The points are integers at least 1 apart inside the box (0..16)^3, so that a post-pass leaves them alone."""
import numpy as np


def _mesh(points, tris):
    return np.asarray(points, dtype=np.float64).reshape(-1, 3), np.asarray(tris, dtype=np.int32).reshape(-1, 3)


def tetrahedron():
    return _mesh([(2, 2, 2), (10, 2, 3), (5, 11, 2), (6, 5, 12)], [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)])


def torus_grid(n=4):
    "n x n periodic quad grid, every quad cut in two"
    P = [(8 + (4 + 2 * np.cos(2 * np.pi * j / n)) * np.cos(2 * np.pi * i / n), 8 + (4 + 2 * np.cos(2 * np.pi * j / n)) * np.sin(2 * np.pi * i / n),
          8 + 2 * np.sin(2 * np.pi * j / n)) for i in range(n) for j in range(n)]
    T = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = n * i + j, n * ((i + 1) % n) + j, n * ((i + 1) % n) + (j + 1) % n, n * i + (j + 1) % n
            T += [(a, b, c), (a, c, d)]
    return _mesh(P, T)


_INNER = [(11, 8), (10, 11), (6, 11), (5, 8), (6, 5), (10, 5)]       # ring 1..6 -> vertices 0..5
_OUTER = [(14, 8), (11, 14), (5, 14), (2, 8), (5, 2), (11, 2)]       # ring 1'..6' -> vertices 6..11


def annulus():
    "flat ring of 12 triangles between two hexagons"
    P = [(x, y, 8) for x, y in _INNER + _OUTER]
    T = []
    for i in range(6):
        j = (i + 1) % 6
        T += [(6 + i, 6 + j, i), (6 + j, j, i)]
    return _mesh(P, T)


def moebius():
    "5 triangles (i, i+1, i+2) mod 5: the edges {i, i+1} are shared, the edges {i, i+2} are one boundary loop"
    return _mesh([(2, 2, 2), (10, 3, 4), (12, 11, 3), (5, 13, 9), (1, 7, 12)], [(i, (i + 1) % 5, (i + 2) % 5) for i in range(5)])


def book():
    "three triangles on the edge 0-1"
    return _mesh([(2, 2, 2), (2, 2, 8), (8, 2, 5), (2, 8, 5), (8, 8, 5)], [(0, 1, 2), (1, 0, 3), (0, 1, 4)])


def pinched_wheel():
    "the annulus, a centre a = 12 and the fan sectors (a,1,2), (a,2,3), (a,4,5), (a,5,6) of the inner ring"
    P, T = annulus()
    P = np.vstack([P, [(8, 8, 8)]])
    fans = [(12, 0, 1), (12, 1, 2), (12, 3, 4), (12, 4, 5)]
    return _mesh(P, np.vstack([T, fans]))


def two_touching_triangles():
    "two triangles that share vertex 0 only: two components"
    return _mesh([(8, 8, 8), (2, 3, 4), (3, 9, 2), (13, 12, 11), (12, 4, 14)], [(0, 1, 2), (0, 3, 4)])


def edge_components(tris):
    "triangle labels of the shared-edge graph, ids in ascending order of the smallest triangle index"
    T = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    lab = list(range(len(T)))
    edges = {}
    for t, row in enumerate(T):
        for k in range(3):
            edges.setdefault(frozenset((int(row[k]), int(row[(k + 1) % 3]))), []).append(t)
    changed = True
    while changed:
        changed = False
        for ts in edges.values():
            m = min(lab[t] for t in ts)
            for t in ts:
                if lab[t] != m:
                    lab[t], changed = m, True
    ids = {r: i for i, r in enumerate(sorted(set(lab)))}
    return np.array([ids[r] for r in lab], dtype=np.int32)
