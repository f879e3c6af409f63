"""numpy restatement of the rim caps (include/contourist_hip.h, section "rim caps"), written from the header text: plain loops over the
faces, squares and face-triangles, dictionaries instead of tables.  Test infrastructure only."""
import numpy as np

FACE_NAMES = ("-x", "+x", "-y", "+y", "-z", "+z")
ALL_FACES = 0x3F
SIDE_BELOW = 1            # flag bit 0 of cx_cap3d
COUNT_KEYS = ("n_lattice_vertices", "n_cap_triangles", "n_missing_crossings", "n_rim_crossings")
# in-plane axes (u, w) of the faces of axis 0, 1, 2: u < w, the diagonal of a square runs from (a, b) to (a + 1, b + 1)
IN_PLANE = ((1, 2), (0, 2), (0, 1))


def inside_mask(grid, value, side):
    "a lattice point is inside iff !(f < v) for 'above', f < v for 'below' (every supported sample type converts to float64 exactly)"
    low = np.asarray(grid).astype(np.float64) < float(value)
    return low if side == "below" else ~low


def reversed_face(face, side):
    """The corners of a face-triangle are numbered counter-clockwise in the (u, w) plane, i.e. around e_u x e_w = +x, -y, +z.  The march's
    normals point from f < v to f >= v: into the solid {f >= v} and out of the solid {f < v}.  'above' therefore wants the cap's normal
    to point INTO the array (+axis on a low face, -axis on a high one), 'below' out of it."""
    axis, high = face >> 1, face & 1
    natural_positive = axis != 1
    want_positive = (not high) if side == "above" else bool(high)
    return natural_positive != want_positive


def cap(grid, value, faces, side, keys0):
    """-> dict(keys (C,) uint32: the cap vertices in ascending key, triangles (K, 3) int32: indices into the Level-0 vertices followed by
    the cap vertices, counts (4,) int64)"""
    assert side in ("above", "below")
    A = np.asarray(grid)
    n = A.shape
    ins = inside_mask(A, value, side)
    keys0 = np.asarray(keys0, dtype=np.int64)
    index0 = {int(k): i for i, k in enumerate(keys0)}
    nv = len(keys0)

    def lin(p):
        return (p[0] * n[1] + p[1]) * n[2] + p[2]

    def crossing(p, q):
        lo, hi = (p, q) if lin(p) < lin(q) else (q, p)
        d = 4 * (hi[0] - lo[0]) + 2 * (hi[1] - lo[1]) + (hi[2] - lo[2])
        return lin(lo) * 8 + d

    out = []                     # triples of keys
    for face in range(6):
        if not (faces >> face) & 1:
            continue
        axis = face >> 1
        u, w = IN_PLANE[axis]
        fixed = n[axis] - 1 if face & 1 else 0
        rev = reversed_face(face, side)

        def P(a, b):
            p = [0, 0, 0]
            p[axis], p[u], p[w] = fixed, a, b
            return tuple(p)
        for a in range(n[u] - 1):
            for b in range(n[w] - 1):
                for c in ((P(a, b), P(a + 1, b), P(a + 1, b + 1)), (P(a, b), P(a + 1, b + 1), P(a, b + 1))):
                    bit = [bool(ins[p]) for p in c]
                    m = sum(bit)
                    pieces = []
                    if m == 3:
                        pieces = [(lin(c[0]) * 8, lin(c[1]) * 8, lin(c[2]) * 8)]
                    elif m == 1:
                        i = bit.index(True)
                        j, k = (i + 1) % 3, (i + 2) % 3
                        pieces = [(lin(c[i]) * 8, crossing(c[i], c[j]), crossing(c[i], c[k]))]
                    elif m == 2:
                        i = bit.index(False)
                        j, k = (i + 1) % 3, (i + 2) % 3
                        x = crossing(c[i], c[j])
                        pieces = [(x, lin(c[j]) * 8, lin(c[k]) * 8), (x, lin(c[k]) * 8, crossing(c[k], c[i]))]
                    for t in pieces:
                        out.append((t[0], t[2], t[1]) if rev else t)
    used = set(k for t in out for k in t)
    lattice = sorted(k for k in used if k & 7 == 0)
    crossings = [k for k in used if k & 7]
    missing = sorted(k for k in crossings if k not in index0)
    cap_keys = sorted(lattice + missing)
    index = dict(index0)
    index.update({k: nv + r for r, k in enumerate(cap_keys)})
    tris = np.array([[index[k] for k in t] for t in out], dtype=np.int32).reshape(-1, 3)
    counts = np.array([len(lattice), len(out), len(missing), len(crossings)], dtype=np.int64)
    return dict(keys=np.array(cap_keys, dtype=np.uint32), triangles=tris, counts=counts)


def points(grid, value, keys, grid64=None):
    "float64 positions of vertices given by their keys: the post-pass's formula (a lattice point, direction 0, is itself)"
    A = np.asarray(grid).astype(np.float64) if grid64 is None else np.asarray(grid64, dtype=np.float64)
    n = A.shape
    keys = np.asarray(keys, dtype=np.int64)
    l, d = keys >> 3, keys & 7
    i, r = np.divmod(l, n[1] * n[2])
    j, k = np.divmod(r, n[2])
    q = np.stack([i, j, k], axis=1).astype(np.float64)
    db = np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1).astype(np.float64)
    flat = A.reshape(-1)
    l2 = l + ((d >> 2) & 1) * n[1] * n[2] + ((d >> 1) & 1) * n[2] + (d & 1)
    f0, f1 = flat[l], flat[l2]
    owner_low = ~(f0 > f1)
    flow, fhigh = np.where(owner_low, f0, f1), np.where(owner_low, f1, f0)
    den = 1.0 * (fhigh - flow)
    ok = ~(np.abs(den) <= 1e-8)
    ratio = np.where(ok, (float(value) - flow) / np.where(ok, den, 1.0), 0.5)
    low = np.where(owner_low[:, None], q, q + db)
    high = np.where(owner_low[:, None], q + db, q)
    return low + ratio[:, None] * (high - low)


def capped_level0(grid, value, faces, side, keys0, xyz0, tris0):
    "the concatenation the post-pass starts from: (keys, points, triangles, cap dict)"
    C = cap(grid, value, faces, side, keys0)
    keys = np.concatenate([np.asarray(keys0, dtype=np.int64), C["keys"].astype(np.int64)])
    xyz = np.concatenate([np.asarray(xyz0, dtype=np.float64).reshape(-1, 3), points(grid, value, C["keys"]).reshape(-1, 3)])
    tris = np.concatenate([np.asarray(tris0, dtype=np.int64).reshape(-1, 3), C["triangles"].astype(np.int64)])
    return keys, xyz, tris, C


def edge_uses(tris):
    """directed-edge census of a triangle list -> (boundary edges, non-manifold edges, incoherent edges, Euler number): an undirected edge
    used once is a boundary edge, more than twice non-manifold, twice in the SAME direction incoherent"""
    tris = np.asarray(tris, dtype=np.int64).reshape(-1, 3)
    if not len(tris):
        return 0, 0, 0, 0
    a = np.concatenate([tris[:, 0], tris[:, 1], tris[:, 2]])
    b = np.concatenate([tris[:, 1], tris[:, 2], tris[:, 0]])
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    und, inv, cnt = np.unique(np.stack([lo, hi], axis=1), axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    fwd = np.bincount(inv, weights=(a < b).astype(np.float64), minlength=len(und)).astype(np.int64)
    boundary = int(np.count_nonzero(cnt == 1))
    nonmanifold = int(np.count_nonzero(cnt > 2))
    incoherent = int(np.count_nonzero((cnt == 2) & (fwd != 1)))
    euler = len(np.unique(tris)) - len(und) + len(tris)
    return boundary, nonmanifold, incoherent, euler


def signed_volume(points_xyz, tris):
    "sum of det(p0, p1, p2) / 6: the enclosed volume of a closed mesh, positive when the normals point outward"
    P = np.asarray(points_xyz, dtype=np.float64)[np.asarray(tris, dtype=np.int64).reshape(-1, 3)]
    return float(np.sum(np.einsum("ij,ij->i", P[:, 0], np.cross(P[:, 1], P[:, 2]))) / 6.0)


def faces_mask(faces):
    "'all', a mask, or a list of the names '-x', '+x', '-y', '+y', '-z', '+z' -> the 6-bit mask"
    if isinstance(faces, str) and faces == "all":
        return ALL_FACES
    if isinstance(faces, (int, np.integer)):
        return int(faces)
    m = 0
    for name in faces:
        m |= 1 << FACE_NAMES.index(name)
    return m


def wind_low_to_high(grid, value, pairs, xyz, tris):
    """the triangles of a Level-0 mesh wound as the device march winds them: normal from f < value to f >= value.  Inside a Kuhn
    tetrahedron the interpolant is linear, a triangle's normal is parallel to its gradient, and every one of its vertices sits on a
    lattice edge from a low to a high corner: the sign of normal . (sum of those edge vectors) decides."""
    A = np.asarray(grid).astype(np.float64)
    pr = np.asarray(pairs, dtype=np.int64).reshape(-1, 6)
    t = np.array(tris, dtype=np.int64).reshape(-1, 3)
    if not len(t):
        return t
    fa, fb = A[pr[:, 0], pr[:, 1], pr[:, 2]], A[pr[:, 3], pr[:, 4], pr[:, 5]]
    a_low = (fa < value) & ~(fb < value)
    up = np.where(a_low[:, None], pr[:, 3:] - pr[:, :3], pr[:, :3] - pr[:, 3:]).astype(np.float64)
    P = np.asarray(xyz, dtype=np.float64)
    nrm = np.cross(P[t[:, 1]] - P[t[:, 0]], P[t[:, 2]] - P[t[:, 0]])
    flip = np.einsum("ij,ij->i", nrm, up[t].sum(axis=1)) < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


# ---- the fields of the tests ---------------------------------------------------------------------------------------------------------
def _ijk(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def _noise(shape, seed, passes=0):
    """noise kept away from the isovalue 0.  passes == 0: white, magnitudes in [0.05, 1), random signs -- every topological case of a
    face-triangle, no weld.  passes > 0: white noise averaged over neighbours that many times per axis, normalised, then pushed 0.05 away
    from zero -- a surface of many sheets with a tenth of the triangles"""
    rng = np.random.default_rng(seed)
    if not passes:
        return (rng.uniform(0.05, 1.0, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    A = rng.normal(size=tuple(n + passes for n in shape))
    for _ in range(passes):
        A = (A[1:] + A[:-1]) / 2
        A = (A[:, 1:] + A[:, :-1]) / 2
        A = (A[:, :, 1:] + A[:, :, :-1]) / 2
    A = A / np.abs(A).max()
    return (A + np.where(A < 0, -0.05, 0.05)).astype(np.float32)


SPHERE_OFF = (3.17, 10.17, 9.83)     # the cut sphere of the closedness assertions: off the lattice (see field())


def field(name):
    """-> (samples, isovalue).  'sphere_exact' is the sphere of radius 9 about (3, 10, 10) in 21^3 as written: the lattice has points at
    distance exactly 9 from that centre, (0, 4, 4) on the rim among them, so it is the parity-only case with a rim sample EQUAL to the
    isovalue; the closedness assertions need every sample 1e-3 away from the isovalue and use 'sphere', the same sphere with its centre
    moved off the lattice by (0.17, 0.17, -0.17)."""
    if name == "constant":
        return np.zeros((5, 4, 3), dtype=np.float32), 1.0
    if name == "plane":
        return _ijk((8, 6, 5))[0].astype(np.float32), 2.5
    if name in ("sphere", "sphere_exact"):
        c = SPHERE_OFF if name == "sphere" else (3.0, 10.0, 10.0)
        I, J, K = _ijk((21, 21, 21))
        return (9.0 - np.sqrt((I - c[0]) ** 2 + (J - c[1]) ** 2 + (K - c[2]) ** 2)).astype(np.float32), 0.0
    if name == "noise_14x20x26":
        return _noise((14, 20, 26), 11), 0.0
    if name == "noise_33x17x66":
        return _noise((33, 17, 66), 12, passes=14), 0.0
    if name == "noise_u8":
        A, _v = field("noise_14x20x26")
        return np.clip(np.round(128.0 + 100.0 * A.astype(np.float64)), 0, 255).astype(np.uint8), 127.5
    raise KeyError(name)


FIELDS = ("constant", "plane", "sphere", "sphere_exact", "noise_14x20x26", "noise_33x17x66", "noise_u8")
MASKS = (0x3F, 0x01, 0x2A, 0)
