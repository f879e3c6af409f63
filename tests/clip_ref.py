"""numpy restatement of the section "clipping" of include/contourist_hip.h (cx_level1_clip_plane / _scalars), written from the
header's text: inside / outside, the two cutting rules, one cut vertex per mesh edge, the order of the cut vertices, the d == 0
rule, keys, the map and the carried normals.  The clean rule and the orientation step are not restated here (oracle/postpass.py has
the first; the second only reverses whole components, which the tests read from the components' `flipped`).  A helper of the
tests, not a conftest."""
import numpy as np

NO_CLEAN, KEEP_BELOW, NORMALS = 1, 2, 4


def plane_scalars(P, normal):
    "s = n0*x + n1*y + n2*z, left to right, every operation rounded once (numpy fuses nothing)"
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    n = [float(x) for x in normal]
    return n[0] * P[:, 0] + n[1] * P[:, 1] + n[2] * P[:, 2]


def clip(P, T, s, threshold=0.0, keep_below=False, normals=None):
    """the mesh cx_level1_clip_scalars leaves with CX_CLIP_NO_CLEAN, before the orientation step turns whole components:
    dict(points, triangles (device order, windings of the rule), keys, map_lo_hi, map_t, normals, source (the source triangle of every
    output triangle), raw_points / raw_triangles / raw_source: the list handed to the tail -- the clean rule's input --,
    n_cut_vertices, n_cut_triangles, n_nonfinite, n_on_cut, d, cut_lo_hi, cut_t)"""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    V, nt = len(P), len(T)
    assert len(s) == V
    with np.errstate(invalid="ignore", over="ignore"):
        d = (threshold - s) if keep_below else (s - threshold)
    fin = np.isfinite(d)
    inside = fin & (d >= 0)
    zero = inside & (d == 0)
    bad = ~np.all(fin[T], axis=1) if nt else np.zeros(0, dtype=bool)
    IN = inside[T] if nt else np.zeros((0, 3), dtype=bool)
    nin = IN.sum(axis=1)
    # ---- the cut corners: edge k of triangle t joins corners k and (k+1)%3; it is cut when one end is inside with d != 0 and the other outside
    A, B = T, np.roll(T, -1, axis=1)
    a_in, b_in = inside[A], inside[B]
    cut = ((a_in & ~b_in & ~zero[A]) | (b_in & ~a_in & ~zero[B])) & ~bad[:, None] if nt else np.zeros((0, 3), dtype=bool)
    tt, kk = np.nonzero(cut)                                 # ascending 3t + k
    corner = 3 * tt + kk
    lo, hi = np.minimum(A[tt, kk], B[tt, kk]), np.maximum(A[tt, kk], B[tt, kk])
    ekey = lo * max(V, 1) + hi
    uniq, inv = np.unique(ekey, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(len(uniq), np.iinfo(np.int64).max)
    np.minimum.at(first, inv, corner)
    order = np.argsort(first)                                # cut vertices by the smallest corner number on their edge
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[order] = np.arange(len(uniq))
    C = len(uniq)
    cut_lo, cut_hi = (uniq // max(V, 1))[order], (uniq % max(V, 1))[order]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        cut_t = d[cut_lo] / (d[cut_lo] - d[cut_hi])
        cut_p = P[cut_lo] + cut_t[:, None] * (P[cut_hi] - P[cut_lo])
    cutidx = -np.ones((nt, 3), dtype=np.int64)
    cutidx[tt, kk] = V + rank[inv]

    def c(t, e, a):
        "c(a, b) on edge e of triangle t, a the inside end: vertex a itself where d[a] == 0"
        return np.where(zero[a], a, cutidx[t, e])
    rows, src, sub = [], [], []
    sel = np.nonzero((nin == 3) & ~bad)[0]
    rows.append(T[sel]); src.append(sel); sub.append(np.zeros(len(sel), dtype=np.int64))
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        t1 = np.nonzero((nin == 1) & IN[:, i] & ~bad)[0]     # corner i inside: edge i joins i and j, edge k joins k and i
        vi = T[t1, i]
        rows.append(np.stack([vi, c(t1, i, vi), c(t1, k, vi)], axis=1)); src.append(t1); sub.append(np.zeros(len(t1), dtype=np.int64))
        t2 = np.nonzero((nin == 2) & ~IN[:, i] & ~bad)[0]    # corner i outside
        vj, vk = T[t2, j], T[t2, k]
        cji, cki = c(t2, i, vj), c(t2, k, vk)
        rows.append(np.stack([cji, vj, vk], axis=1)); src.append(t2); sub.append(np.zeros(len(t2), dtype=np.int64))
        rows.append(np.stack([cji, vk, cki], axis=1)); src.append(t2); sub.append(np.ones(len(t2), dtype=np.int64))
    rows, src, sub = np.concatenate(rows), np.concatenate(src), np.concatenate(sub)
    ok = (rows[:, 0] != rows[:, 1]) & (rows[:, 0] != rows[:, 2]) & (rows[:, 1] != rows[:, 2])       # two equal indices: dropped
    rows, src, sub = rows[ok], src[ok], sub[ok]
    o = np.lexsort((sub, src))                               # source-triangle order, the first of a pair before the second
    rows, src = rows[o], src[o]
    assert rows.min(initial=0) >= 0
    raw_points = np.concatenate([P, cut_p]) if C else P.copy()
    used = np.unique(rows.reshape(-1))
    vnew = -np.ones(V + C + 1, dtype=np.int64)
    vnew[used] = np.arange(len(used))
    old = used < V
    m_lo, m_hi, m_t = used.copy(), used.copy(), np.zeros(len(used))
    r = used[~old] - V
    m_lo[~old], m_hi[~old], m_t[~old] = cut_lo[r], cut_hi[r], cut_t[r]
    out = dict(points=raw_points[used], triangles=vnew[rows].astype(np.int32), keys=used.astype(np.uint32),
               map_lo_hi=np.stack([m_lo, m_hi], axis=1).astype(np.int32), map_t=m_t, source=src, raw_points=raw_points, raw_triangles=rows,
               raw_source=src, n_cut_vertices=C, n_cut_triangles=len(np.unique(tt)), n_nonfinite=int(bad.sum()), n_on_cut=int(zero.sum()), d=d,
               cut_lo_hi=np.stack([cut_lo, cut_hi], axis=1), cut_t=cut_t)
    if normals is not None:
        N = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
        u = 1.0 - cut_t
        x = u[:, None] * N[cut_lo] + cut_t[:, None] * N[cut_hi]
        length = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
        cn = np.zeros((C, 3))
        nz = length > 0.0
        cn[nz] = x[nz] / length[nz][:, None]
        out["normals"] = (np.concatenate([N, cn]) if C else N.copy())[used]
        out["cut_normals"] = cn
    return out


def carry(values, lo_hi, t):
    "(1 - t) * values[lo] + t * values[hi]"
    values = np.asarray(values)
    t = np.asarray(t, dtype=np.float64).reshape((-1,) + (1,) * (values.ndim - 1))
    return (1.0 - t) * values[lo_hi[:, 0]] + t * values[lo_hi[:, 1]]


def unflip(tris, tri_labels, flipped):
    "rows as they were before the orientation step reversed the components with flipped == 1: (a,b,c) <- (c,b,a)"
    t = np.array(tris, dtype=np.int64).reshape(-1, 3)
    f = np.asarray(flipped)[np.asarray(tri_labels)].astype(bool) if len(t) else np.zeros(0, dtype=bool)
    t[f] = t[f][:, ::-1]
    return t


def area(P, T):
    P, T = np.asarray(P, dtype=np.float64), np.asarray(T, dtype=np.int64).reshape(-1, 3)
    if len(T) == 0:
        return 0.0
    return float(np.sum(np.linalg.norm(np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]]), axis=1)) / 2.0)


def euler_and_boundary(T):
    "(V - E + F over the vertices in use, number of edges used by one triangle) of the whole mesh"
    T = np.asarray(T, dtype=np.int64).reshape(-1, 3)
    if len(T) == 0:
        return 0, 0
    a, b = T.ravel(), np.roll(T, -1, axis=1).ravel()
    key = np.minimum(a, b) * (int(T.max()) + 1) + np.maximum(a, b)
    _u, mult = np.unique(key, return_counts=True)
    return len(np.unique(T)) - len(mult) + len(T), int(np.count_nonzero(mult == 1))
