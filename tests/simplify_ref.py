"""numpy / Python-int restatement of the section "simplification" of include/contourist_hip.h (cx_level1_simplify), written from
the header's text: clusters, exact means, the order, the remap, the degenerate and duplicate rules, the carried normals.  The
clean rule and the orientation step are not restated here (oracle/postpass.py has the first; the second only reverses whole
components, which the tests read from the components' `flipped`).  A helper of the tests, not a conftest."""
import numpy as np

NO_CLEAN, ACROSS_COMPONENTS, COUNT_ONLY, NORMALS = 1, 2, 4, 8


def q_of(corner):
    "52 - ceil(log2(max corner + 2)), in integers"
    m = int(max(int(c) for c in corner)) + 2
    return 52 - (m - 1).bit_length()


def cell_box(corner, cell3):
    "(first cell, number of cells) per axis of the grid box: floor(-1 / c) .. floor((corner + 1) / c)"
    corner = np.asarray(corner, dtype=np.float64)
    c = np.asarray(cell3, dtype=np.float64)
    kmin = np.floor(-1.0 / c)
    kn = np.floor((corner + 1.0) / c) - kmin + 1.0
    return kmin.astype(np.int64), kn.astype(np.int64)


def admissible(corner, cell3):
    kmin, kn = cell_box(corner, cell3)
    return int(kn[0]) * int(kn[1]) * int(kn[2]) < 2 ** 31


def vertex_labels(tris, nv):
    """(triangle labels, vertex labels) as cx_level1_component_labels defines them: components of the graph "triangles that share an
    undirected edge", ids by smallest triangle index; a vertex takes the smallest id among its triangles, -1 when unused"""
    T = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    nt = len(T)
    lab = np.arange(nt)
    if nt:
        a, b = T, np.roll(T, -1, axis=1)
        keys = (np.minimum(a, b) * nv + np.maximum(a, b)).ravel()
        t = np.repeat(np.arange(nt), 3)
        order = np.argsort(keys, kind="stable")
        keys, t = keys[order], t[order]
        same = keys[1:] == keys[:-1]
        ea, eb = t[:-1][same], t[1:][same]
        while True:
            m = np.minimum(lab[ea], lab[eb])
            new = lab.copy()
            np.minimum.at(new, ea, m)
            np.minimum.at(new, eb, m)
            while True:
                jump = new[new]
                if np.array_equal(jump, new):
                    break
                new = jump
            if np.array_equal(new, lab):
                break
            lab = new
    roots = np.unique(lab)
    rank = np.zeros(nt + 1, dtype=np.int64)
    rank[roots] = np.arange(len(roots))
    tl = rank[lab].astype(np.int32)
    vl = np.full(nv, np.iinfo(np.int32).max, dtype=np.int32)
    for k in range(3):
        np.minimum.at(vl, T[:, k], tl)
    vl[vl == np.iinfo(np.int32).max] = -1
    return tl, vl


def clusters(P, vlab, corner, cell3, by_component=True):
    """-> (cluster id per old vertex (-1: dropped), first member per cluster, cell per vertex (V,3)).  Cluster ids ascend with the first
    member, the cluster's smallest old vertex index."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    c = np.broadcast_to(np.asarray(cell3, dtype=np.float64), (3,))
    kmin, kn = cell_box(corner, c)
    k = np.floor(P / c).astype(np.int64) if len(P) else np.zeros((0, 3), dtype=np.int64)
    kc = np.clip(k - kmin, 0, kn - 1)                   # a vertex outside the grid box counts to the box's nearest cell
    lin = (kc[:, 0] * kn[1] + kc[:, 1]) * kn[2] + kc[:, 2]
    vlab = np.asarray(vlab, dtype=np.int64)
    key = ((vlab if by_component else 0 * vlab) << 31) | lin
    valid = np.nonzero(vlab >= 0)[0]
    cid = -np.ones(len(P), dtype=np.int64)
    if len(valid) == 0:
        return cid, np.zeros(0, dtype=np.int64), kc + kmin
    _u, first_pos, inv = np.unique(key[valid], return_index=True, return_inverse=True)
    first = valid[first_pos]                            # smallest member of every cluster (np.unique: first occurrence)
    order = np.argsort(first)
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    cid[valid] = rank[inv.reshape(-1)]
    return cid, first[order], kc + kmin


def remap_triangles(T, cid):
    "-> (remapped rows (T,3), mask: three distinct clusters, none dropped)"
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    M = cid[T] if len(T) else np.zeros((0, 3), dtype=np.int64)
    ok = np.all(M >= 0, axis=1) & (M[:, 0] != M[:, 1]) & (M[:, 0] != M[:, 2]) & (M[:, 1] != M[:, 2])
    return M, ok


def exact_means(P, cid, ncl, corner, q, only=None):
    """(positions (ncl,3), clamped coordinates): X = rint(clamp(x) * 2^q) added as Python integers, float(sum) / float(n) * 2^-q.
    only: the cluster ids to compute (the others stay NaN)"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    hi = np.asarray(corner, dtype=np.float64) + 1.0
    Pc = np.minimum(np.maximum(P, -1.0), hi)
    members = cid >= 0
    clamped = int(np.count_nonzero(Pc[members] != P[members]))
    X = np.rint(Pc * 2.0 ** q).astype(np.int64)
    out = np.full((ncl, 3), np.nan)
    order = np.argsort(cid, kind="stable")
    order = order[cid[order] >= 0]
    bounds = np.searchsorted(cid[order], np.arange(ncl + 1))
    todo = range(ncl) if only is None else only
    inv = 2.0 ** -q
    for c in todo:
        rows = X[order[bounds[c]:bounds[c + 1]]]
        n = len(rows)
        for a in range(3):
            s = sum(int(x) for x in rows[:, a])         # exact
            out[c, a] = float(s) / float(n) * inv       # float(int): rounded once, to nearest even
    return out, clamped


def carried_normals(Nsrc, cid, ncl):
    "normalised sums of rint(n * 2^30) per cluster; (0,0,0) for a zero sum"
    Nsrc = np.asarray(Nsrc, dtype=np.float64).reshape(-1, 3)
    I = np.rint(np.clip(Nsrc, -1.0, 1.0) * 2.0 ** 30).astype(np.int64)
    S = np.zeros((ncl, 3), dtype=np.int64)
    m = cid >= 0
    np.add.at(S, cid[m], I[m])                          # (|sum| < members * 2^30: exact in int64)
    x = S.astype(np.float64)
    length = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    out = np.zeros((ncl, 3))
    nz = length > 0.0
    out[nz] = x[nz] / length[nz][:, None]
    return out


def scaled_normals(N, delta):
    "what cx_level1_normals(delta3) serves after a simplification: normalize(N / delta)"
    x = np.asarray(N, dtype=np.float64) / np.asarray(delta, dtype=np.float64)
    length = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    out = x.copy()
    nz = length > 0.0
    out[nz] = x[nz] / length[nz][:, None]
    return out


def simplify(P, T, corner, cell, by_component=True, normals=None, vlab=None):
    """the mesh cx_level1_simplify leaves with CX_SIMPLIFY_NO_CLEAN, before the orientation step turns whole components:
    dict(points, triangles (device order, windings of the input), keys, map, normals, q, n_clusters, n_distinct, clamped, old_triangle,
    raw_points / raw_triangles / raw_old: the clusters' mesh before unused vertices are compacted away -- the clean rule's input)"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    if vlab is None:
        vlab = vertex_labels(T, len(P))[1]
    cell3 = np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,))
    assert admissible(corner, cell3)
    q = q_of(corner)
    cid, first, _k = clusters(P, vlab, corner, cell3, by_component)
    ncl = len(first)
    pos, clamped = exact_means(P, cid, ncl, corner, q)
    M, ok = remap_triangles(T, cid)
    n_distinct = int(ok.sum())
    # of several triangles with the same vertex set the one with the smallest old index stays
    alive = np.nonzero(ok)[0]
    if len(alive):
        _s, keep = np.unique(np.sort(M[alive], axis=1), axis=0, return_index=True)
        alive = alive[np.sort(keep)]
    rows = M[alive]
    used = np.unique(rows.reshape(-1))
    vnew = -np.ones(ncl + 1, dtype=np.int64)
    vnew[used] = np.arange(len(used))
    out = dict(points=pos[used], triangles=vnew[rows].astype(np.int32), keys=first[used].astype(np.uint32),
               map=np.where(cid >= 0, vnew[cid], -1).astype(np.int32), q=q, n_clusters=ncl, n_distinct=n_distinct, clamped=clamped,
               old_triangle=alive, raw_points=pos, raw_triangles=rows, raw_old=alive, cluster=cid, first=first)
    if normals is not None:
        out["normals"] = carried_normals(normals, cid, ncl)[used]
    return out


def unflip(tris, tri_labels, flipped):
    "rows as they were before the orientation step reversed the components with flipped == 1: (a,b,c) <- (c,b,a)"
    t = np.array(tris, dtype=np.int64).reshape(-1, 3)
    f = np.asarray(flipped)[np.asarray(tri_labels)].astype(bool) if len(t) else np.zeros(0, dtype=bool)
    t[f] = t[f][:, ::-1]
    return t


def sphere_mesh(n_lat=24, n_lon=48, radius=9.7, centre=(12.3, 11.6, 12.9)):
    "an analytic sphere: a latitude / longitude mesh with two poles, wound outward; (points, triangles)"
    pts = [(0.0, 0.0, 1.0)]
    for i in range(1, n_lat):
        th = np.pi * i / n_lat
        for j in range(n_lon):
            ph = 2.0 * np.pi * j / n_lon
            pts.append((np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)))
    pts.append((0.0, 0.0, -1.0))
    P = np.array(pts) * radius + np.asarray(centre)
    ring = lambda i, j: 1 + (i - 1) * n_lon + (j % n_lon)
    tris = []
    for j in range(n_lon):
        tris.append((0, ring(1, j), ring(1, j + 1)))
        tris.append((len(pts) - 1, ring(n_lat - 1, j + 1), ring(n_lat - 1, j)))
    for i in range(1, n_lat - 1):
        for j in range(n_lon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            tris.append((a, c, d))
            tris.append((a, d, b))
    return P, np.array(tris, dtype=np.int32)
