"""numpy restatement of the "topology" definitions of include/contourist_hip.h, from (triangles, triangle labels) only.

topology(tris, tlab) -> (table, loops, loop vertices) in the layouts of _ffi.TOPOLOGY_DTYPE / _ffi.LOOP_DTYPE."""
import collections

import numpy as np

TOPOLOGY_DTYPE = np.dtype([("triangles", "<i8"), ("vertices", "<i8"), ("edges", "<i8"), ("boundary_edges", "<i8"), ("nonmanifold_edges", "<i8"),
                           ("euler", "<i8"), ("boundary_loops", "<i4"), ("genus", "<i4"), ("nonsimple_loops", "<i4"), ("reserved", "<i4")])
LOOP_DTYPE = np.dtype([("component", "<i4"), ("simple", "<i4"), ("first", "<u4"), ("count", "<u4")])


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def topology(tris, tlab):
    T = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    lab = np.asarray(tlab, dtype=np.int64).reshape(-1)
    nt = len(T)
    nc = int(lab.max()) + 1 if nt else 0
    table = np.zeros(nc, dtype=TOPOLOGY_DTYPE)
    if nt == 0:
        return table, np.zeros(0, dtype=LOOP_DTYPE), np.zeros(0, dtype=np.int32)
    tail, head = T.ravel(), np.roll(T, -1, axis=1).ravel()              # use e = 3 t + k runs tail -> head
    ulab = np.repeat(lab, 3)
    key = np.minimum(tail, head) * (int(T.max()) + 1) + np.maximum(tail, head)
    _u, first, inv, mult = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    elab = ulab[first]                                                  # (all uses of one edge carry one label)
    table["triangles"] = np.bincount(lab, minlength=nc)
    table["vertices"] = np.bincount(np.unique(np.stack([ulab, tail], axis=1), axis=0)[:, 0], minlength=nc)
    table["edges"] = np.bincount(elab, minlength=nc)
    table["boundary_edges"] = np.bincount(elab[mult == 1], minlength=nc)
    table["nonmanifold_edges"] = np.bincount(elab[mult >= 3], minlength=nc)
    table["euler"] = table["vertices"] - table["edges"] + table["triangles"]
    # boundary edges in ascending 3 t + k; union-find: linked when two of one component share a vertex
    be = np.nonzero(mult[inv.reshape(-1)] == 1)[0]
    parent = list(range(len(be)))
    at = {}                                                             # (component, vertex) -> boundary edges there
    for i, e in enumerate(be):
        for v in (int(tail[e]), int(head[e])):
            at.setdefault((int(ulab[e]), v), []).append(i)
    for members in at.values():
        for i in members[1:]:
            a, b = _find(parent, members[0]), _find(parent, i)
            parent[max(a, b)] = min(a, b)
    roots = [_find(parent, i) for i in range(len(be))]                  # the root is the smallest member: ids in its order
    ids = {r: l for l, r in enumerate(sorted(set(roots)))}
    edges_of = [[] for _ in ids]
    for i, r in enumerate(roots):
        edges_of[ids[r]].append(i)
    loops, verts = np.zeros(len(ids), dtype=LOOP_DTYPE), []
    for l, members in enumerate(edges_of):
        c = int(ulab[be[members[0]]])
        ends = [v for i in members for v in (int(tail[be[i]]), int(head[be[i]]))]
        simple = all(n == 2 for n in collections.Counter(ends).values()) and all(tail[be[i]] != head[be[i]] for i in members)
        loops[l] = (c, int(simple), len(verts), len(members))
        if simple:                                                      # walk from the smallest edge in its own direction
            i, v, seen = members[0], int(tail[be[members[0]]]), 0
            while seen < len(members):
                verts.append(v)
                v = int(head[be[i]]) if int(tail[be[i]]) == v else int(tail[be[i]])
                i = [j for j in at[(c, v)] if j != i][0]
                seen += 1
        else:
            verts.extend(int(tail[be[i]]) for i in members)
        table["boundary_loops"][c] += 1
        table["nonsimple_loops"][c] += 0 if simple else 1
    twice = 2 - table["euler"] - table["boundary_loops"]
    ok = (table["nonmanifold_edges"] == 0) & (twice >= 0) & (twice % 2 == 0)
    table["genus"] = np.where(ok, twice // 2, -1)
    return table, loops, np.asarray(verts, dtype=np.int32)
