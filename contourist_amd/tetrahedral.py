"""3-D isosurfaces by marching tetrahedra on MI355X -- host-side mirror of the reference's
`contourist/tetrahedral.py` (Delta3DContour :50-87, TriangulatedIsosurfaces :89-101,
Grid3DContour :104-107, GridContour3d :514-621).

Same class names, constructor arguments, methods and return conventions as the reference; the
work happens in hand-written HIP kernels behind the C ABI (include/contourist_hip.h):

    search_for_endpoints()        -> Level-0 march on the device (crossing search, active voxels,
                                     tetrahedra classification, edge interpolation, triangle emit)
    get_points_and_triangles()    -> device post-passes (weld, tiny collapse, clean, orient) and
                                     one download; returns (points, triangles)

Differences a caller can observe (see DESIGN.md "Boundary"):
  * points is a (V,3) float64 ndarray and triangles a (T,3) int32 ndarray (rows sorted); both
    index / iterate like the reference's list of arrays / sorted list of tuples.
  * the march is a dense scan: EVERY component of the isosurface inside the grid is returned,
    not only those reachable from the seed segments.
  * flatten=True (serial LP decimation)
    are not offered on the device path and raise NotImplementedError.
"""
import itertools

import numpy as np

from . import _ffi
from . import grid_field
from . import surface_geometry

# cube corners, Kuhn tetrahedra and the 26-neighbourhood, in the reference's order
# (tetrahedral.py:20-47): corner c = 4*di + 2*dj + dk, tetrahedra = monotone paths A..H.
CUBE = np.array(list(itertools.product((0, 1), repeat=3)), dtype=int)
_A, _B, _C, _D, _E, _F, _G, _H = (tuple(c) for c in CUBE)
TETRAHEDRA = np.array([[_A, _H, _B, _D], [_A, _H, _D, _C], [_A, _H, _C, _G],
                       [_A, _H, _G, _E], [_A, _H, _E, _F], [_A, _H, _F, _B]], dtype=int)
OFFSETS = np.array([o for o in itertools.product((-1, 0, 1), repeat=3) if any(o)], dtype=int)

_DEFAULT_DEVICE = [0]


def set_default_device(device):
    _DEFAULT_DEVICE[0] = int(device)


class GridContour3d(object):
    """Device-backed counterpart of GridContour3d (tetrahedral.py:514-621) working in GRID coordinates.

    corner   = voxels per axis (the reference's `corner`); the sample array has corner+1 per axis.
    samples  = dense fp32 array (numpy) or torch tensor on the GPU, shape corner+1.
    """

    # One extraction addresses its samples and edges with 32-bit ids: 2^29 samples at most (include/contourist_hip.h, cx_grid_upload).
    # A larger volume -- 1024^3 fp32 is 4 GB of the 288 GB of an MI355X -- is marched slab by slab along axis 0 on the same context
    # (each slab with one plane of its upper neighbour, global edge ids, as the ranks of distributed.level1_slabs do) and
    # post-processed as ONE mesh.  Lowered by the tests to force the slab path on small volumes.
    MAX_SAMPLES_PER_EXTRACTION = 1 << 29

    def __init__(self, corner, samples, value, segment_endpoints=None, linear_interpolate=True,
                 callback=None, device=None, diagonal="cpython310", context=None, voxel_range=None, function=None, samples64=None):
        self.corner = np.array(corner, dtype=int)
        assert self.corner.shape == (3,), "dimension must be 3"
        if segment_endpoints is not None:
            for (p1, p2) in segment_endpoints:
                assert len(p1) == 3
                assert len(p2) == 3
        if not linear_interpolate and function is None:
            raise NotImplementedError("linear_interpolate=False re-evaluates the function between the lattice points "
                                      "(tetrahedral.py:488-505): it needs the callable, a sample array is not enough")
        self.dimension = 3
        self.linear_interpolate = bool(linear_interpolate)
        self.function = function      # f(i, j, k) in the lattice coordinates of `samples` (linear_interpolate=False only)
        self._f_broadcasts = None
        self.end_points = segment_endpoints
        self.voxel_range = voxel_range    # in_range box of the seeded growth (lo, hi); None = the whole array
        self.keep_in_range = False        # True: every voxel of the box is kept, the end points only add seed voxels outside it
        self.origin = (0, 0, 0)           # lattice coordinates of sample (0,0,0) in the reference's grid (hash order of the diagonals)
        self.grid_shift = 0               # the sample array starts this many lattice steps before the reference's grid
        self.value = float(value)
        self.callback = callback
        self.flatten = False
        self.smooth = None
        self.samples = samples
        self.samples64 = samples64    # float64 originals of a callable's samples (the reference interpolates on these), or None
        shape = tuple(int(n) for n in samples.shape)
        assert samples64 is None or tuple(samples64.shape) == shape
        assert shape == tuple(int(c) + 1 for c in self.corner), (shape, self.corner)
        self.shape = shape
        self.device = _DEFAULT_DEVICE[0] if device is None else int(device)
        self.flags = {"cpython310": _ffi.CX_DIAG_CPYTHON310, "canonical": _ffi.CX_DIAG_CANONICAL}[diagonal]
        self._ctx = context
        self._counts = None
        self._post = None
        self._cap = None              # (face mask, side) of cap_rim(), or None
        self.cap_counts = None

    # -- device plumbing ----------------------------------------------------------------------------
    def context(self):
        if self._ctx is None:
            self._ctx = _ffi.Context(self.device)
        return self._ctx

    def _bind_grid(self):
        ctx = self.context()
        s = self.samples
        if grid_field._is_torch(s):
            assert s.is_cuda and s.is_contiguous() and _ffi.native_dtype(s.dtype), \
                "device samples must be a contiguous tensor on the GPU of a supported dtype (%s)" % ", ".join(_ffi.DTYPE_CODES)
            ctx.adopt_device_grid(s.data_ptr(), self.shape, keepalive=s, dtype=s.dtype)
        else:
            ctx.upload_grid_native(s)
        ctx.shadow_grid_f64(self.samples64)

    def _in_slabs(self):
        "more samples than one extraction addresses: the volume goes through the device slab by slab"
        return int(np.prod(self.shape, dtype=np.int64)) > int(self.MAX_SAMPLES_PER_EXTRACTION)

    def _slab_planes(self):
        "planes of axis 0 per slab, so that a slab plus its halo plane stays within one extraction"
        per_plane = int(self.shape[1]) * int(self.shape[2])
        planes = int(self.MAX_SAMPLES_PER_EXTRACTION) // per_plane - 1
        if planes < 2:
            raise ValueError("a plane of %d x %d samples leaves no room for a slab of two planes and its halo in one extraction "
                             "(%d samples)" % (self.shape[1], self.shape[2], int(self.MAX_SAMPLES_PER_EXTRACTION)))
        return planes

    @staticmethod
    def _slab_bounds(n0, planes):
        """[(i0, i1), ...]: consecutive ranges of planes covering [0, n0), `planes` each (every slab but the last is marched with plane
        i1 as its halo); a single trailing plane joins the slab before it (alone it would hold no voxel; planes + 1 still fit one
        extraction, that slab has no halo)"""
        bounds, at = [], 0
        while at < n0:
            end = min(n0, at + planes)
            if n0 - end == 1:
                end = n0
            bounds.append((at, end))
            at = end
        return bounds

    def _post_in_slabs(self, clean=True):
        """Level 0 slab by slab + Level 1 of the assembled mesh (the single-process form of distributed.level1_slabs: same slabs,
        same global edge ids, same post-pass on ONE mesh, so components, weld buckets and the max-x rule see the whole surface).
        Leaves the Level-1 mesh in the context (download_level1 / level1_torch) and returns the post-pass counts."""
        from . import distributed
        if (self.end_points is not None and len(self.end_points)) or self.voxel_range is not None or not self.linear_interpolate \
                or tuple(self.origin) != (0, 0, 0) or self.grid_shift:
            raise NotImplementedError("a volume of more than %d samples is marched in slabs: exhaustive search, linear interpolation and "
                                      "an array without a rim only (no end points, no voxel range)" % int(self.MAX_SAMPLES_PER_EXTRACTION))
        ctx = self.context()
        s, s64 = self.samples, self.samples64
        on_device = grid_field._is_torch(s)
        if on_device:
            assert s.is_cuda and s.is_contiguous() and _ffi.native_dtype(s.dtype), \
                "device samples must be a contiguous tensor on the GPU of a supported dtype (%s)" % ", ".join(_ffi.DTYPE_CODES)
        else:   # slabs of a supported type are uploaded in that type
            s = np.asarray(s)
            s = _ffi.native_array(s) if _ffi.native_dtype(s.dtype) else np.ascontiguousarray(s, dtype=np.float32)
        n0 = int(self.shape[0])
        planes = self._slab_planes()
        parts = []
        totals = dict(n_cells=0, n_vertices=0, n_triangles=0, n_border_voxels=0)
        bounds = self._slab_bounds(n0, planes)
        for (i0, i1) in bounds:
            has_halo = i1 < n0
            local = s[i0:i1 + (1 if has_halo else 0)]
            ctx.set_origin(i0, 0, 0)
            if on_device:
                ctx.adopt_device_grid(local.data_ptr(), tuple(int(n) for n in local.shape), keepalive=s, dtype=s.dtype)
            else:
                ctx.upload_grid_native(local)
            ctx.shadow_grid_f64(None if s64 is None else s64[i0:i1 + (1 if has_halo else 0)])
            counts = ctx.extract3d(self.value, self.flags)
            _xyz32, keys, tris = ctx.download_level0(counts)
            xyz = ctx.level0_points_f64(counts)            # global coordinates (the origin is added before interpolating)
            parts.append(distributed.local_to_global(xyz, keys, tris, tuple(local.shape), i0, i1 - i0, has_halo, True))
            for k in totals:
                totals[k] += int(counts[k])
        ctx.set_origin(0, 0, 0)
        keys, xyz, tris = distributed.assemble(parts)
        self._slab_counts = dict(totals, n_slabs=len(parts), n_vertices=int(len(keys)), n_triangles=int(len(tris)))
        ctx.set_reference_corner((0, 0, 0))
        return ctx.postprocess3d_mesh(xyz, tris, [int(c) for c in self.corner], (0 if clean else 1) | _ffi.CX_MESH_OF_THE_MARCH, self.smooth or 0.0)

    def march(self, force=False):
        "Level 0 on the device (idempotent). returns the counts dict."
        if self._in_slabs():
            raise NotImplementedError("a volume of more than %d samples has no single Level-0 extraction: get_points_and_triangles() "
                                      "marches it in slabs" % int(self.MAX_SAMPLES_PER_EXTRACTION))
        if self._counts is None or force:
            self._bind_grid()
            self.context().set_origin(*self.origin)
            self._counts = self.context().extract3d(self.value, self.flags)
            self._post = None
        return self._counts

    def level0(self):
        """Level-0 mesh as host arrays: dict(xyz (V,3) f32 grid coords, keys (V,) u32 edge ids,
        triangles (T,3) i32 wound low->high, counts)."""
        counts = self.march()
        xyz, keys, tris = self.context().download_level0(counts)
        return dict(xyz=xyz, keys=keys, triangles=tris, counts=counts)

    # -- reference API -------------------------------------------------------------------------------
    def extract_surface_geometry(self, clean=True):
        "SurfaceGeometry of the welded, cleaned and oriented mesh in grid coordinates (tetrahedral.py:604-621)"
        if self.flatten:
            raise NotImplementedError("flatten=True (lp_tools decimation) is outside the device path")
        if self._in_slabs():
            if self.smooth:
                assert self.smooth > 0 and self.smooth <= 1
            ctx = self.context()
            if self._post is None:
                self._post = self._post_in_slabs(clean)
            pts, tris = ctx.download_level1(self._post)
            return surface_geometry.SurfaceGeometry._from_device(pts, tris, ctx)
        self.march()
        if self.flatten:
            raise NotImplementedError("flatten=True (lp_tools decimation) is outside the device path")
        if self.smooth:
            assert self.smooth > 0 and self.smooth <= 1
        ctx = self.context()
        if self._post is None:
            # explicit end points restrict the result to the components the reference's breadth-first search
            # reaches from them (tetrahedral.py:396-463); None = every component (exhaustive search_for_endpoints)
            if self.end_points is not None and len(self.end_points):
                self.seeded = ctx.select_seeded(self.end_points, self.voxel_range, self.keep_in_range)
            if self.voxel_range is not None:   # the array has a margin: Level-1 scales of the reference's own grid
                lo, hi = self.voxel_range
                ctx.set_reference_corner([int(h) - int(l) for l, h in zip(lo, hi)])
            else:
                ctx.set_reference_corner((0, 0, 0))
            if self._cap is not None:
                self._post = self._postprocess_capped(ctx, clean)
            elif self.linear_interpolate:
                self._post = ctx.postprocess3d(0 if clean else 1, self.smooth or 0.0)
            else:
                self._post = self._postprocess_refined(ctx, clean)
        # an array with a rim (grid_shift, origin = -grid_shift) is post-processed in the reference's own lattice
        # coordinates on the device (weld buckets truncate towards zero there as in the reference): nothing to shift back
        pts, tris = ctx.download_level1(self._post)
        return surface_geometry.SurfaceGeometry._from_device(pts, tris, ctx)

    def _ensure_post(self, clean=True):
        "Level 1 on the device, left there (no download); returns the context"
        if self._in_slabs():
            ctx = self.context()
            if self._post is None:
                self._post = self._post_in_slabs(clean)
            return ctx
        self.march()
        ctx = self.context()
        if self._post is None:
            if self.end_points is not None and len(self.end_points):
                self.seeded = ctx.select_seeded(self.end_points, self.voxel_range, self.keep_in_range)
            if self.voxel_range is not None:
                lo, hi = self.voxel_range
                ctx.set_reference_corner([int(h) - int(l) for l, h in zip(lo, hi)])
            else:
                ctx.set_reference_corner((0, 0, 0))
            if self._cap is not None:
                self._post = self._postprocess_capped(ctx, clean)
            else:
                self._post = ctx.postprocess3d(0 if clean else 1, self.smooth or 0.0) if self.linear_interpolate else self._postprocess_refined(ctx, clean)
        return ctx

    # -- rim caps: close the surface where the rim of the array cuts it open --------------------------------------
    def _cap_refusal(self):
        "why this maker takes no cap, or None"
        if self._in_slabs():
            return "a volume marched in slabs has no single extraction whose rim could be capped"
        if self.end_points is not None and len(self.end_points):
            return "end points select components of the surface: a cap closes the whole surface, not a selection of it"
        if self.voxel_range is not None or self.grid_shift or tuple(self.origin) != (0, 0, 0):
            return "a voxel_range (an array carrying a margin) has its rim outside the grid"
        if not self.linear_interpolate:
            return "linear_interpolate=False moves the crossings off the march's piecewise-linear surface: the flat caps would not meet them"
        if self.smooth:
            return "smooth moves the rim's vertices out of the faces of the array"
        return None

    def cap_rim(self, faces="all", side="above"):
        """Close the surface where the rim of the sampled array cuts it open (include/contourist_hip.h, "rim caps"): every later
        get_points_and_triangles(), components(), topology(), write_mesh(), simplify() and clip() serves march + cap, a closed mesh
        whose components() volume is that of {f >= value} (side="above") or {f < value} ("below") under the march's interpolant.
        faces: "all", a 6-bit mask, or a list of "-x", "+x", "-y", "+y", "-z", "+z".  Returns the cap's counts (_ffi.CAP_KEYS).
        cap_rim(None) undoes it.  Normals and curvature are not served for a capped mesh (a crease runs along the rim)."""
        if faces is None:
            self._cap, self.cap_counts, self._post = None, None, None
            return None
        mask, flags = _ffi.cap_faces_mask(faces), _ffi.cap_side_flags(side)
        why = self._cap_refusal()
        if why:
            raise NotImplementedError("cap_rim: " + why)
        self.march()
        self.cap_counts = self.context().cap3d(mask, side)
        self._cap = (mask, "below" if flags else "above")
        self._post = None
        return dict(self.cap_counts)

    def _postprocess_capped(self, ctx, clean):
        why = self._cap_refusal()
        if why:
            raise NotImplementedError("cap_rim: " + why)
        self.cap_counts = ctx.cap3d(*self._cap)        # (idempotent: built again only after a new extraction)
        return dict(ctx.postprocess3d_capped(0 if clean else 1), capped=True, carried_normals=False)

    # -- vertex attributes: normals from the field's gradient, a second grid sampled at the vertices -------------
    def _attr_checks(self):
        if not self.linear_interpolate:
            raise NotImplementedError("vertex normals and sampled values need linear_interpolate=True: refined points are not "
                                      "crossings {edge, fraction} of the resident sample array")
        if self._in_slabs():
            raise NotImplementedError("vertex normals and sampled values of a volume marched in slabs are not available: the "
                                      "assembled mesh's vertices are not edge crossings of one resident array")

    def level0_normals(self, device=False):
        "(V,4) float32 {nx, ny, nz, |g|} next to level0(): the unit gradient direction and the gradient's length per vertex record"
        counts = self.march()
        return self.context().level0_normals(counts, None, device)

    def level0_values(self, field, device=False):
        "(V,) float32: `field` (array or device tensor of the grid's shape, marched in its own type) at the vertices of level0()"
        counts = self.march()
        return self.context().level0_sample(counts, field, device)

    def vertex_normals(self, clean=True, device=False, delta=None):
        """(V,3) float64 unit normals in grid coordinates; row i belongs to row i of get_points_and_triangles()[0] and agrees with
        the winding of its triangles.  delta: world spacing per axis (the world normal is g / delta, normalised)."""
        self._attr_checks()
        ctx = self._ensure_post(clean)
        return ctx.level1_normals(self._post, delta, device)

    def level0_curvature(self, device=False):
        "(V,4) float32 {mean, gauss, k1, k2} next to level0(): mean, Gaussian and principal curvatures per vertex record (grid units)"
        counts = self.march()
        return self.context().level0_curvature(counts, None, device)

    def vertex_curvature(self, clean=True, device=False, delta=None):
        """(V,4) float64 {mean, gauss, k1, k2} in grid units (1/voxel, 1/voxel^2); row i belongs to row i of
        get_points_and_triangles()[0] and is signed like vertex_normals(): a sphere whose normals point outwards has mean > 0.
        delta: world spacing per axis (curvature in world units).  Not available after simplify()."""
        self._attr_checks()
        ctx = self._ensure_post(clean)
        return ctx.level1_curvature(self._post, delta, device)

    def vertex_values(self, field, clean=True, device=False):
        "(V,) float64: `field` (array or device tensor of the grid's shape, any supported dtype) at the vertices of get_points_and_triangles()"
        self._attr_checks()
        ctx = self._ensure_post(clean)
        return ctx.level1_sample(self._post, field, device)

    # -- components of the welded mesh: labels, per-component measures, filtering ----------------------------------
    def components(self, clean=True, mins=None, delta=None, device=False):
        """the connected components of get_points_and_triangles() as a numpy structured array (_ffi.COMPONENT_DTYPE: triangles,
        vertices, area, volume, centroid, bbox_lo, bbox_hi, flipped, closed, first_triangle), measured on the device; component
        c is row c.  mins / delta: world = grid * delta + mins (grid coordinates without them).
        device=True: (table, triangle labels, vertex labels), the labels as torch tensors on the GPU in device order."""
        ctx = self._ensure_post(clean)
        table = ctx.level1_components(mins, delta)
        if device:
            return (table,) + tuple(ctx.level1_component_labels(device=True))
        return table

    def component_labels(self, clean=True, device=False):
        """(triangle labels (T,), vertex labels (V,)) int32: the component id of every triangle, and per vertex the smallest id
        among its triangles' components (-1 for a vertex no triangle uses).  Host: triangle labels in the order of the sorted
        rows get_points_and_triangles() returns; device=True: torch tensors in device order, next to
        get_points_and_triangles(device=True)."""
        ctx = self._ensure_post(clean)
        if device:
            return ctx.level1_component_labels(device=True)
        tl, vl = ctx.level1_component_labels()
        _pts, tris = ctx.download_level1(self._post)
        return tl[surface_geometry.row_order(tris)], vl

    def topology(self, clean=True, device=False):
        """the topology of the components of get_points_and_triangles() as a numpy structured array (_ffi.TOPOLOGY_DTYPE:
        triangles, vertices, edges, boundary_edges, nonmanifold_edges, euler, boundary_loops, genus, nonsimple_loops), counted on
        the device; row c is component c of components().  device=True: a torch int32 tensor (nc, 16) on the GPU."""
        return self._ensure_post(clean).level1_topology(device)

    def boundary_loops(self, clean=True, device=False, mins=None, delta=None):
        """the boundary curves of the mesh, where the array's rim or a seeded range cut it open: (loops, vertices, points).
        loops: a numpy structured array (_ffi.LOOP_DTYPE: component, simple, first, count); vertices: int32 row numbers of
        get_points_and_triangles()[0], loop l in vertices[first : first + count], in cyclic order for a simple loop; points:
        a list with one (count, 3) float64 array per loop (grid coordinates; world = grid * delta + mins when given).
        device=True: (loops, vertices) as torch int32 tensors on the GPU, the loops as (L, 4) rows."""
        ctx = self._ensure_post(clean)
        if device:
            return ctx.level1_boundary_loops(device=True)
        loops, verts = ctx.level1_boundary_loops()
        return loops, verts, _loop_points(ctx.download_level1(self._post)[0], loops, verts, mins, delta)

    def keep_components(self, mask=None, largest=None, min_triangles=None, min_area=None, closed=None, clean=True, genus=None,
                        boundary_loops=None):
        """drop components of the mesh ON THE DEVICE: mask (one entry per component), largest=k (most triangles, ties by id),
        min_triangles, min_area (grid coordinates), closed, genus and boundary_loops (an int or an inclusive (lo, hi) range, read
        from topology()); the selectors combine with AND.  Afterwards
        get_points_and_triangles(), vertex_normals(), vertex_values(), write_mesh(), components() give the filtered mesh
        (until the next march).  -> dict(n_vertices, n_triangles, n_components)"""
        ctx = self._ensure_post(clean)
        topo = ctx.level1_topology() if (genus is not None or boundary_loops is not None) else None
        keep = surface_geometry.select_components(ctx.level1_components(), mask, largest, min_triangles, min_area, closed, topo, genus, boundary_loops)
        counts = ctx.level1_keep_components(keep)
        self._post = dict(self._post, **counts)
        return counts

    # -- simplification by vertex clustering on the device (the reference's flatten=True is LP decimation: not this) -------------
    def simplify(self, cell=None, target_triangles=None, by_component=True, clean=True, normals="auto"):
        """reduce the mesh ON THE DEVICE by vertex clustering (cx_level1_simplify): the vertices of one cell of a lattice of `cell`
        voxels (a scalar or three), per component unless by_component=False, become one vertex at their exact mean.
        target_triangles=N instead of cell: the smallest scalar cell a bisection over [1, max(corner)] finds (dry runs only, at
        most 16, down to 1/16 voxel) whose mesh has no more than N triangles; ValueError if the largest cell does not get there.
        normals: True carries the vertex normals over (vertex_normals() serves them), False drops them, "auto" carries them where
        vertex_normals() is available.  Afterwards get_points_and_triangles(), vertex_normals(), components(), keep_components()
        and write_mesh() give the simplified mesh until the next march; vertex_values() raises NotImplementedError.
        -> dict(n_vertices, n_triangles, n_components, n_clusters, cell, clamped)"""
        if (cell is None) == (target_triangles is None):
            raise ValueError("exactly one of cell and target_triangles is needed")
        ctx = self._ensure_post(clean)
        if normals == "auto":
            try:
                self._attr_checks()
                normals = bool(self._post.get("carried_normals", True))
            except NotImplementedError:
                normals = False
        counts = _simplify_on(ctx, cell, target_triangles, by_component, clean, bool(normals), max(int(c) for c in self.corner), self)
        self._post = dict(self._post, carried_normals=bool(normals), **{k: counts[k] for k in ("n_vertices", "n_triangles", "n_components")})
        return counts

    def simplify_map(self, device=False):
        "(V_before,) int32: the new index of every vertex of the mesh before the last simplify(), -1 where it went away"
        return self.context().level1_simplify_map(getattr(self, "_simplify_n_old", 0), device)      # (none yet: the library's CX_ERR_STATE)

    # -- clipping by a plane, a box or a scalar field on the device --------------------------------------------------------------
    def clip(self, plane=None, box=None, field=None, scalars=None, value=0.0, keep="above", clean=True, normals="auto", mins=None, delta=None):
        """cut the mesh open ON THE DEVICE (cx_level1_clip_*); exactly one of
        plane=(normal3, offset): keeps n.p >= offset, in grid coordinates, or in world coordinates when mins / delta are given
            (converted on the host: n_grid = n * delta, offset_grid = offset - n.mins);
        box=(lo3, hi3): six plane clips in the fixed order -x, +x, -y, +y, -z, +z, stopping early when the mesh is empty; the counts
            of cut vertices, cut triangles, non-finite and on-cut vertices are summed over them, and clip_map() then describes
            the LAST of them only;
        field=: a second grid of the samples' shape, scalars = vertex_values(field) kept on the device, keeps field >= value (not
            available on a derived mesh -- after simplify() or clip());
        scalars=: a (V,) array or device tensor, converted to float64, keeps scalars >= value.
        keep="below" keeps the other side (not for a box).  Triangles the cut crosses are cut; a vertex exactly on the cut is not
        duplicated.  normals: as for simplify().  Afterwards every reader gives the clipped mesh, whose boundary_loops() are the cut
        curves; vertex_values() and vertex_curvature() raise NotImplementedError.
        -> dict(n_vertices, n_triangles, n_components, n_cut_vertices, n_cut_triangles, n_nonfinite, n_on_cut)"""
        spec = _clip_args(plane, box, field, scalars, keep, mins, delta)
        ctx = self._ensure_post(clean)
        if normals == "auto":
            try:
                self._attr_checks()
                normals = bool(self._post.get("carried_normals", True))
            except NotImplementedError:
                normals = False
        counts = _clip_on(ctx, spec, value, keep, clean, bool(normals))
        self._post = dict(self._post, carried_normals=bool(normals), **{k: counts[k] for k in ("n_vertices", "n_triangles", "n_components")})
        return counts

    def clip_map(self, device=False):
        "(lo_hi (V',2) int32, t (V',) float64) of the last clip(): output vertex i lies on the edge lo_hi[i] of the mesh before it, at t[i]"
        return self.context().level1_clip_map(device)

    def clip_values(self, values):
        "a per-vertex array (numpy or torch) of the mesh before the last clip() carried across it: (1-t)*values[lo] + t*values[hi]"
        return _clip_values(values, self.context())

    def write_mesh(self, path, fmt="ply", mins=None, delta=None, clean=True):
        """the welded, cleaned, oriented mesh as a binary file written STRAIGHT FROM THE DEVICE BUFFERS (cx_level1_write: no
        (points, triangles) arrays on the host) -- the step every caller of the reference takes next (html_demo.py:118-161).
        fmt "ply" | "gltf_bin" | "ply_normals" | "gltf_bin_normals"; mins / delta: world = grid * delta + mins.  Faces in device order
        (the Python API sorts rows)."""
        if fmt.endswith("_normals"):
            self._attr_checks()
        ctx = self._ensure_post(clean)
        return ctx.write_level1(path, fmt, mins, delta)

    # -- linear_interpolate=False (tetrahedral.py:488-505) ------------------------------------------------------
    def _feval(self, P):
        "function at the rows of P (N,3), float64: one broadcast call if the function allows it, else one call per row"
        P = np.asarray(P, dtype=np.float64).reshape(-1, 3)
        if len(P) == 0:
            return np.zeros(0)
        if self._f_broadcasts is not False:
            try:
                out = np.asarray(self.function(P[:, 0], P[:, 1], P[:, 2]), dtype=np.float64)
                if out.shape != (len(P),):
                    self._f_broadcasts = False
                elif self._f_broadcasts is None:     # first time: spot-check the broadcast result against scalar calls
                    probe = [0, len(P) // 2, len(P) - 1]
                    self._f_broadcasts = all(abs(out[k] - float(self.function(*P[k]))) <= 1e-12 * max(1.0, abs(out[k])) for k in probe)
                if self._f_broadcasts:
                    return out
            except Exception:
                self._f_broadcasts = False
        return np.array([float(self.function(*row)) for row in P], dtype=np.float64)

    def _refined_points(self, keys):
        """the reference's float64 crossing points with its regula-falsi refinement: contour_pair_interpolation
        (tetrahedral.py:471-512) with linear_interpolate == False, iterations = 5, for every crossing edge at once"""
        lo, hi = unpack_edge_ids(keys, self.shape)
        return refined_crossing_points(self._feval, self.value, lo, hi)

    def _postprocess_refined(self, ctx, clean):
        """Level 1 on refined points: the Level-0 mesh comes to the host, its points are replaced by the reference's
        refined ones (the caller's function is Python), and the same device post-pass runs on the result"""
        L = self.level0()
        keys, tris = L["keys"].astype(np.int64), L["triangles"].astype(np.int64)
        tkeep, vkeep = ctx.seeded_masks(L["counts"])
        tris = tris[tkeep]
        used = np.zeros(len(keys), dtype=bool)
        used[tris.ravel()] = True
        used &= vkeep | used
        ids = np.nonzero(used)[0]
        order = ids[np.argsort(keys[ids], kind="stable")]                    # ascending edge id: index == priority
        renum = -np.ones(len(keys), dtype=np.int64)
        renum[order] = np.arange(len(order))
        pts = self._refined_points(keys[order])
        if self.grid_shift and len(pts):
            pts = pts - float(self.grid_shift)          # the reference's own lattice coordinates (weld buckets, output)
        if self.voxel_range is not None:
            lo, hi = self.voxel_range
            corner = [int(h) - int(l) for l, h in zip(lo, hi)]
        else:
            corner = [int(c) for c in self.corner]
        return ctx.postprocess3d_mesh(pts, renum[tris], corner, (0 if clean else 1) | _ffi.CX_MESH_OF_THE_MARCH, self.smooth or 0.0)

    def get_points_and_triangles(self, clean=True, device=False):
        """(grid_points (V,3) float64, triangles (T,3) int32 sorted rows)  (tetrahedral.py:528-552).
        device=True: the same mesh as torch tensors ON THE GPU (points float64, triangles int32 in device order, each row wound
        as the host rows are) -- no download; for consumers that live on the device (cx_level1_device_ptrs)."""
        if device:
            ctx = self._ensure_post(clean)
            if self.callback:
                self.callback(self)
            return ctx.level1_torch(copy=True)
        geometry = self.extract_surface_geometry(clean)
        if self.callback:
            self.callback(self)
        return (geometry.vertices, geometry.oriented_triangles)

    extract_points_and_triangles = get_points_and_triangles

    # lazily derived views of the reference's bookkeeping (tetrahedral.py:158-169)
    @property
    def interpolated_contour_pairs(self):
        "{((i,j,k) low, (i,j,k) high): grid xyz} as the reference keeps it -- host side, for inspection only"
        L = self.level0()
        lo, hi = unpack_edge_ids(L["keys"], self.shape)
        S = np.asarray(self.samples if not grid_field._is_torch(self.samples) else self.samples.cpu().float().numpy())
        swap = S[tuple(lo.T)] > S[tuple(hi.T)]
        a = np.where(swap[:, None], hi, lo)
        b = np.where(swap[:, None], lo, hi)
        return {(tuple(int(x) for x in p), tuple(int(x) for x in q)): np.array(c, dtype=float)
                for p, q, c in zip(a, b, L["xyz"])}


def _simplify_on(ctx, cell, target_triangles, by_component, clean, normals, max_corner, owner):
    "simplify() of the three isosurface classes on the context that holds the mesh; owner gets _simplify_n_old and _simplify_search"
    flags = (0 if clean else _ffi.CX_SIMPLIFY_NO_CLEAN) | (0 if by_component else _ffi.CX_SIMPLIFY_ACROSS_COMPONENTS)
    owner._simplify_search = []          # [(cell, triangles with three distinct indices)] of the dry runs, in the order they ran
    if target_triangles is not None:
        n = int(target_triangles)

        def dry(c):
            got = ctx.level1_simplify(c, flags | _ffi.CX_SIMPLIFY_COUNT_ONLY)["n_distinct"]
            owner._simplify_search.append((float(c), int(got)))
            return got
        lo, hi = 1.0, float(max(1, max_corner))
        reached = dry(hi)
        if reached > n:
            raise ValueError("target_triangles=%d is out of reach: the largest cell (%g voxels) still leaves %d triangles" % (n, hi, reached))
        if hi > lo and dry(lo) <= n:
            hi = lo
        while len(owner._simplify_search) < 16 and hi - lo >= 1.0 / 16.0:
            mid = 0.5 * (lo + hi)
            if dry(mid) <= n:
                hi = mid          # (the smallest cell found so far that stays within n)
            else:
                lo = mid
        cell = hi
    n_old = ctx.level1_device_ptrs()[2]
    counts = ctx.level1_simplify(cell, flags | (_ffi.CX_SIMPLIFY_NORMALS if normals else 0))
    owner._simplify_n_old = int(n_old)
    return {k: counts[k] for k in _ffi.SIMPLIFY_KEYS}


def _clip_args(plane, box, field, scalars, keep, mins=None, delta=None):
    """the source of a clip() checked and brought into grid coordinates, before anything touches the device:
    ("planes", [(normal3, offset), ...]) | ("field", field) | ("scalars", scalars)"""
    given = [name for name, v in (("plane", plane), ("box", box), ("field", field), ("scalars", scalars)) if v is not None]
    if len(given) != 1:
        raise ValueError("exactly one of plane, box, field and scalars is needed (got %s)" % (", ".join(given) or "none"))
    if keep not in ("above", "below"):
        raise ValueError('keep must be "above" or "below"')
    d = np.ones(3) if delta is None else np.asarray(delta, dtype=np.float64).reshape(3)
    m = np.zeros(3) if mins is None else np.asarray(mins, dtype=np.float64).reshape(3)

    def to_grid(n, offset):
        n = np.asarray(n, dtype=np.float64).reshape(3)
        offset = float(offset)
        if not (np.all(np.isfinite(n)) and np.isfinite(offset)) or not np.any(n != 0.0):
            raise ValueError("a plane needs a finite normal that is not zero and a finite offset")
        return n * d, offset - float(np.dot(n, m))
    if plane is not None:
        normal, offset = plane
        return "planes", [to_grid(normal, offset)]
    if box is not None:
        if keep != "above":
            raise ValueError('a box keeps its inside: keep="below" is not available for it')
        lo, hi = (np.asarray(x, dtype=np.float64).reshape(3) for x in box)
        planes = []
        for a in range(3):
            e = np.zeros(3)
            e[a] = 1.0
            planes.append(to_grid(e, lo[a]))
            planes.append(to_grid(-e, -hi[a]))
        return "planes", planes
    return ("field", field) if field is not None else ("scalars", scalars)


def _clip_on(ctx, spec, value, keep, clean, normals):
    "clip() of the three isosurface classes on the context that holds the mesh"
    flags = (0 if clean else _ffi.CX_CLIP_NO_CLEAN) | (_ffi.CX_CLIP_KEEP_BELOW if keep == "below" else 0) | (_ffi.CX_CLIP_NORMALS if normals else 0)
    kind, what = spec
    if kind == "field":
        counts = ctx.level1_clip_field(what, value, flags)
    elif kind == "scalars":
        counts = ctx.level1_clip_scalars(what, value, flags)
    else:
        counts = None
        for n, offset in what:
            c = ctx.level1_clip_plane(n, offset, flags)
            if counts is not None:
                for k in ("n_cut_vertices", "n_cut_triangles", "n_nonfinite", "n_on_cut"):
                    c[k] += counts[k]
            counts = c
            if counts["n_triangles"] == 0:
                break
    return {k: counts[k] for k in _ffi.CLIP_KEYS}


def _clip_values(values, ctx):
    "(1 - t) * values[lo] + t * values[hi] over the map of the last clip; a torch tensor on the device stays there"
    if hasattr(values, "data_ptr"):
        lo_hi, t = ctx.level1_clip_map(device=values.is_cuda)
        if not values.is_cuda:
            import torch
            lo_hi, t = torch.from_numpy(lo_hi), torch.from_numpy(t)
        lo, hi = lo_hi[:, 0].long(), lo_hi[:, 1].long()
        t = t.to(values.dtype) if values.dtype.is_floating_point else t
    else:
        values = np.asarray(values)
        lo_hi, t = ctx.level1_clip_map()
        lo, hi = lo_hi[:, 0], lo_hi[:, 1]
    if values.ndim > 1:
        t = t.reshape((-1,) + (1,) * (values.ndim - 1))
    return (1.0 - t) * values[lo] + t * values[hi]


def unpack_edge_ids(keys, shape):
    "edge id (lin << 3 | d) -> (lower lattice point (V,3), upper lattice point (V,3)); d == 0 (a lattice-point vertex of a rim cap): both are the point"
    keys = np.asarray(keys).astype(np.int64)
    lin, d = keys >> 3, keys & 7
    i, r = np.divmod(lin, shape[1] * shape[2])
    j, k = np.divmod(r, shape[2])
    lo = np.stack([i, j, k], axis=1)
    hi = lo + np.stack([(d >> 2) & 1, (d >> 1) & 1, d & 1], axis=1)
    return lo, hi


def bisect_endpoints(lattice_function, value, pairs, lo, hi, dropped=None):
    """The bisection of GridContour.find_initial_voxels (tetrahedral.py:408-423) on the host, for end points that lie OUTSIDE the
    sampled array: the reference evaluates its callable wherever the end points are (its own demos pass (20,20,20) on a 12^3
    grid and (100,100,100) in world coordinates, html_demo.py:147-161, 277-282) and halves the lattice segment until the two
    points are neighbours.  Same swaps, same assert, same integer midpoints, the callable in float64.  A pair inside the box
    [lo, hi] per axis is handed on untouched (the device bisects it on the samples, as before); a pair that leaves the box is
    replaced by the neighbouring pair its bisection ends at.  A pair whose bisection ENDS outside the box (the crossing it brackets
    is not in the sampled array, rim included) is left out and appended to `dropped` if given: the reference would emit the
    triangles of that one voxel out there -- evaluating its callable where this build has no samples -- and grow nothing from it
    (in_range, tetrahedral.py:465-469); the device cannot, and refusing the whole call for it (CX_ERR_INVALID, as round 3 did)
    is worse than leaving the stray voxel out.  -> list of (low_point, high_point) int arrays"""
    out = []
    lo, hi = np.asarray(lo), np.asarray(hi)
    for a, b in pairs:
        a, b = np.array(a, dtype=np.int64), np.array(b, dtype=np.int64)
        inside = np.all(a >= lo) and np.all(a <= hi) and np.all(b >= lo) and np.all(b <= hi)
        if inside:
            out.append((a, b))
            continue
        low_point, high_point = a, b
        low_value, high_value = float(lattice_function(*low_point)), float(lattice_function(*high_point))
        if low_value > value or high_value < value:
            low_point, low_value, high_point, high_value = high_point, high_value, low_point, low_value
        assert low_value <= value and high_value >= value, "Bad end points " + repr((low_point, low_value, high_point, high_value, value))
        while np.any(np.abs(low_point - high_point) > 1):
            mid_point = (low_point + high_point) // 2
            if float(lattice_function(*mid_point)) < value:
                low_point = mid_point
            else:
                high_point = mid_point
        if np.all(low_point >= lo) and np.all(low_point <= hi) and np.all(high_point >= lo) and np.all(high_point <= hi):
            out.append((low_point, high_point))
        elif dropped is not None:
            dropped.append((low_point, high_point))
    return out


def Grid3DContour(horizontal_n, vertical_m, forward_l, function, value, segment_endpoints,
                  linear_interpolate=True, callback=None, device=None):
    """Grid3DContour(n, m, l, function, value, segment_endpoints, ...)  (tetrahedral.py:104-107).
    `function(i, j, k)` over grid coordinates is sampled once into a dense (n+1, m+1, l+1) array;
    pass a numpy array / GPU tensor of that shape instead of a callable to skip the sampling."""
    corner = (int(horizontal_n), int(vertical_m), int(forward_l))
    if callable(function):
        g = grid_field.FunctionGrid([0, 0, 0], [c - 0.5 for c in corner], [1, 1, 1], function)
        assert tuple(g.grid_dimensions) == corner
        if segment_endpoints is not None and len(segment_endpoints):
            # explicit end points: the reference does not range-check the voxels it starts from and evaluates the function
            # one lattice step outside the grid (tetrahedral.py:396-441): sample that rim too, grow inside the grid only
            m = 1
            segment_endpoints = bisect_endpoints(function, float(value), segment_endpoints, [-m] * 3, [c + m for c in corner])
            shifted = [(np.asarray(a, dtype=int) + m, np.asarray(b, dtype=int) + m) for (a, b) in segment_endpoints]
            maker = GridContour3d(tuple(c + 2 * m for c in corner), g.dense_samples(margin=m), value, shifted, linear_interpolate, callback,
                                  device, voxel_range=((m, m, m), tuple(c + m for c in corner)),
                                  function=lambda i, j, k: function(i - m, j - m, k - m), samples64=g.dense_samples64(margin=m))
            maker.origin = (-m, -m, -m)
            maker.grid_shift = m
            return maker
        samples = g.dense_samples()
    else:
        samples = function
    return GridContour3d(corner, samples, value, segment_endpoints, linear_interpolate, callback, device,
                         function=function if callable(function) else None,
                         samples64=g.dense_samples64() if callable(function) else None)


class Delta3DContour(object):
    """World-coordinate facade (tetrahedral.py:50-87 on top of triangulated.ContourGrid :79-118)."""

    linear_interpolate = True
    flatten = False
    minimum_ratio = None
    minimum_extent = None
    smooth = None
    device = None

    def __init__(self, function_grid, value, segment_endpoints=None, linear_interpolate=True):
        self.linear_interpolate = linear_interpolate
        self.grid = function_grid
        self.value = value
        self.segment_endpoints = segment_endpoints
        grid_endpoints = None
        if segment_endpoints is not None:
            grid_endpoints = []
            for (start_xy, end_xy) in segment_endpoints:
                # the reference asserts len == 2 here (a 2-D leftover, triangulated.py:96) which makes
                # non-empty 3-D endpoints unusable at HEAD; both 2- and 3-vectors are accepted here.
                assert len(start_xy) == len(end_xy) == self.grid.dimension
                grid_endpoint = self.to_grid_endpoint(start_xy, end_xy)
                if grid_endpoint is not None:
                    grid_endpoints.append(grid_endpoint)
            if len(grid_endpoints) < 1:
                grid_endpoints = None
        self.contour_maker = self.get_contour_maker(grid_endpoints)
        self.grid_values = None

    def to_grid_endpoint(self, start_xy, end_xy):
        "first pair of surrounding lattice points whose values straddle the isovalue (triangulated.py:109-118)"
        grid = self.grid
        value = self.value
        for start_grid in grid.surrounding_vertices(np.array(start_xy, dtype=float)):
            for end_grid in grid.surrounding_vertices(np.array(end_xy, dtype=float)):
                if not np.all(start_grid == end_grid):
                    if (grid.grid_function(*start_grid) - value) * (grid.grid_function(*end_grid) - value) <= 0:
                        return (start_grid, end_grid)
        return None

    def get_contour_maker(self, grid_endpoints, rim=True):
        grid = self.grid
        self.grid_endpoints = grid_endpoints
        if self.flatten:
            raise NotImplementedError("flatten=True (lp_tools decimation) is outside the device path")
        gd = np.array([int(n) for n in grid.grid_dimensions])
        self._grid_shift = 0
        if grid_endpoints and rim and not getattr(grid, "array_backed", False):
            # explicit end points on a callable field: the reference does not range-check its seed voxels and
            # evaluates f one lattice step outside the grid (tetrahedral.py:396-441); sample that rim too and
            # keep the breadth-first growth inside the reference's grid
            m = 1
            grid_endpoints = bisect_endpoints(self._lattice_function(0), float(self.value), grid_endpoints, [-m] * 3, list(gd + m))
            shifted = [(np.asarray(a, dtype=int) + m, np.asarray(b, dtype=int) + m) for (a, b) in grid_endpoints]
            result = GridContour3d(tuple(gd + 2 * m), grid.dense_samples(margin=m), self.value, shifted,
                                   linear_interpolate=self.linear_interpolate, device=self.device,
                                   voxel_range=((m, m, m), tuple(gd + m)), function=self._lattice_function(m),
                                   samples64=grid.dense_samples64(margin=m))
            result.origin = (-m, -m, -m)      # the CPython-order diagonals hash the reference's own lattice coordinates
            result.grid_shift = m
            self._grid_shift = m
        else:
            result = GridContour3d(tuple(gd), grid.dense_samples(), self.value,
                                   grid_endpoints, linear_interpolate=self.linear_interpolate, device=self.device,
                                   function=self._lattice_function(0), samples64=grid.dense_samples64())
        result.flatten = self.flatten
        result.smooth = self.smooth
        return result

    def _lattice_function(self, shift):
        """f over the lattice coordinates of the sample array (which may start `shift` steps before the grid): what
        FunctionGrid.grid_function does (grid_field.py:95-118, world = grid * delta + mins), usable on arrays.
        None for a grid made from a sample array."""
        grid = self.grid
        if getattr(grid, "array_backed", False):
            return None
        mins, delta, f = grid.mins, grid.delta, grid.f

        def lattice_f(i, j, k):
            return f((i - shift) * delta[0] + mins[0], (j - shift) * delta[1] + mins[1], (k - shift) * delta[2] + mins[2])
        return lattice_f

    def write_mesh(self, path, fmt="ply"):
        "binary mesh file in WORLD coordinates straight from the device buffers (GridContour3d.write_mesh)"
        if fmt in ("gltf", "gltf_normals"):
            from . import mesh_io
            return mesh_io.write_gltf_device(self, path, normals=fmt == "gltf_normals")
        return self.contour_maker.write_mesh(path, fmt, self.grid.mins, self.grid.delta)

    def cap_rim(self, faces="all", side="above"):
        "GridContour3d.cap_rim of this isosurface (refused, with the reason, when the maker carries a rim of samples around the grid)"
        return self.contour_maker.cap_rim(faces, side)

    def components(self, clean=True, device=False):
        "GridContour3d.components in WORLD coordinates (areas, volumes, centroids and boxes of the grid's mins and delta)"
        return self.contour_maker.components(clean, self.grid.mins, self.grid.delta, device)

    def component_labels(self, clean=True, device=False):
        "GridContour3d.component_labels of this isosurface"
        return self.contour_maker.component_labels(clean, device)

    def topology(self, clean=True, device=False):
        "GridContour3d.topology of this isosurface"
        return self.contour_maker.topology(clean, device)

    def boundary_loops(self, clean=True, device=False):
        "GridContour3d.boundary_loops of this isosurface, the points in WORLD coordinates"
        return self.contour_maker.boundary_loops(clean, device, self.grid.mins, self.grid.delta)

    def keep_components(self, mask=None, largest=None, min_triangles=None, min_area=None, closed=None, clean=True, genus=None, boundary_loops=None):
        "GridContour3d.keep_components; min_area in WORLD units"
        maker = self.contour_maker
        if min_area is not None:
            topo = self.topology(clean) if (genus is not None or boundary_loops is not None) else None
            keep = surface_geometry.select_components(self.components(clean), mask, largest, min_triangles, min_area, closed, topo, genus, boundary_loops)
            return maker.keep_components(mask=keep, clean=clean)
        return maker.keep_components(mask, largest, min_triangles, None, closed, clean, genus, boundary_loops)

    def simplify(self, cell=None, target_triangles=None, by_component=True, clean=True, normals="auto"):
        "GridContour3d.simplify of this isosurface: `cell` in VOXELS (grid units), a scalar or one per axis"
        return self.contour_maker.simplify(cell, target_triangles, by_component, clean, normals)

    def simplify_map(self, device=False):
        "GridContour3d.simplify_map"
        return self.contour_maker.simplify_map(device)

    def clip(self, plane=None, box=None, field=None, scalars=None, value=0.0, keep="above", clean=True, normals="auto", mins=None, delta=None):
        """GridContour3d.clip of this isosurface; plane and box are in WORLD coordinates (the grid's mins and delta, unless mins /
        delta are given), field an array of the grid's shape (grid_dimensions + 1)"""
        mins = self.grid.mins if mins is None else mins
        delta = self.grid.delta if delta is None else delta
        return self.contour_maker.clip(plane, box, field, scalars, value, keep, clean, normals, mins, delta)

    def clip_map(self, device=False):
        "GridContour3d.clip_map"
        return self.contour_maker.clip_map(device)

    def clip_values(self, values):
        "GridContour3d.clip_values"
        return self.contour_maker.clip_values(values)

    def vertex_normals(self, clean=True, device=False):
        """(V,3) float64 unit normals in WORLD coordinates (the gradient per axis divided by delta, normalised); row i belongs
        to row i of get_points_and_triangles()[0]"""
        return self.contour_maker.vertex_normals(clean, device, delta=self.grid.delta)

    def vertex_curvature(self, clean=True, device=False):
        """(V,4) float64 {mean, gauss, k1, k2} in WORLD units (the grid's delta is passed on); row i belongs to row i of
        get_points_and_triangles()[0], signed like vertex_normals()"""
        return self.contour_maker.vertex_curvature(clean, device, delta=self.grid.delta)

    def vertex_values(self, field, clean=True, device=False):
        """(V,) float64: a second field at the vertices.  `field`: an array or device tensor of the grid's shape
        (grid_dimensions + 1), or -- for a grid made from a callable -- a callable g(x, y, z) in world coordinates, sampled
        by the host on the same lattice as the function (its rim included)."""
        maker = self.contour_maker
        m = int(getattr(self, "_grid_shift", 0))
        if callable(field):
            if getattr(self.grid, "array_backed", False):
                raise ValueError("a callable field needs a grid made from a callable")
            second = grid_field.FunctionGrid(self.grid.mins, self.grid.maxes, self.grid.delta, field)
            field = second.dense_samples(margin=m) if m else second.dense_samples()
        elif m:
            raise NotImplementedError("the sample array carries a rim of %d lattice steps around the grid: hand the second field "
                                      "over as a callable" % m)
        return maker.vertex_values(field, clean, device)

    def search_for_endpoints(self, skip=1):
        """Reference: crossing search over every skip-th lattice point + new contour maker (tetrahedral.py:74-81,
        grid_field.py:64-84).  skip == 1 (the canonical call): the device march contains the exhaustive search and
        every component is returned; `grid_endpoints` is derived lazily from the crossing edges it found.
        skip > 1: the coarse search runs on the dense samples, its segments seed the reference's breadth-first
        growth (cx_select_seeded3d), so components the coarse lattice misses stay out, as in the reference."""
        self._skip = skip
        if skip > 1:
            (maxf, minf, segments) = self.grid.find_contour_crossing_grid_segments(self.value, skip)
            self.grid_values = (minf, maxf)
            # coarse segments lie inside the grid: no rim of extra samples needed (rim=False)
            self.contour_maker = self.get_contour_maker(segments if len(segments) else None, rim=False)
            self.contour_maker.march()
            self.grid_endpoints = segments
            return
        rim = None if getattr(self.grid, "array_backed", False) else self._rim_segments()
        if rim is not None and len(rim):
            # the surface reaches the rim of the grid: the reference starts from every crossing segment without
            # range-checking the voxels it starts from (tetrahedral.py:396-441), so the voxels one step OUTSIDE the grid
            # next to the crossing segments on the rim get triangles too.  One extra sample all around, every voxel of
            # the grid kept, the rim segments as seeds
            self.contour_maker = self.get_contour_maker(rim, rim=True)
            self.contour_maker.keep_in_range = True
        else:
            self.contour_maker = self.get_contour_maker(None)
        if not self.contour_maker._in_slabs():      # (a volume beyond one extraction is marched slab by slab in get_points_and_triangles)
            self.contour_maker.march()
        self.grid_endpoints = _LazyEndpoints(self.contour_maker, skip, getattr(self, "_grid_shift", 0), self.grid.grid_dimensions)

    def _rim_segments(self, shell=2):
        """the crossing lattice segments of find_contour_crossing_grid_segments (grid_field.py:64-84: from every lattice
        point 0 <= p < grid_dimensions to its 7 forward neighbours, strict sign change) that lie within `shell` lattice
        steps of the rim of the grid, IN THE REFERENCE'S ORDER (points in index order, last axis fastest; neighbours in
        the order of surrounding_vertices :52-62, first axis fastest).  None if no segment touches the rim itself.
        The order matters: the reference walks its end points one after the other with one shared `visited` set
        (tetrahedral.py:396-441), and which voxel next to the rim a point picks depends on what was visited before."""
        gd = np.array([int(n) for n in self.grid.grid_dimensions])
        S = np.asarray(self.grid.dense_samples_host(), dtype=np.float64)     # vertices 0 .. gd inclusive
        return rim_crossing_segments(S, gd, float(self.value), shell)

    def get_points_and_triangles(self, device=False):
        """(points in world coordinates, triangles)  (tetrahedral.py:83-87).  device=True: torch tensors on the GPU -- the world
        transform grid * delta + mins (grid_field.py:89-93) is applied there too; nothing comes to the host."""
        if device:
            import torch
            (grid_points, triangles) = self.contour_maker.get_points_and_triangles(device=True)
            delta = torch.as_tensor(np.asarray(self.grid.delta, dtype=np.float64), device=grid_points.device)
            mins = torch.as_tensor(np.asarray(self.grid.mins, dtype=np.float64), device=grid_points.device)
            return (grid_points * delta + mins, triangles)
        (grid_points, triangles) = self.contour_maker.get_points_and_triangles()      # (the maker undoes its own shift)
        points = self.grid.from_grid_coordinates(grid_points) if len(grid_points) else np.zeros((0, 3))
        return (points, triangles)


class _LazyEndpoints(object):
    "sequence of (vertex0, vertex1) crossing lattice segments, materialised on first use"

    def __init__(self, maker, skip, shift=0, grid_dimensions=None):
        self._maker, self._skip, self._list = maker, skip, None
        self._shift, self._gd = int(shift), grid_dimensions

    def _get(self):
        if self._list is None:
            L = self._maker.level0()
            lo, hi = unpack_edge_ids(L["keys"], self._maker.shape)
            if self._shift:      # the array carries a rim of extra samples: back to the grid's own lattice
                lo, hi = lo - self._shift, hi - self._shift
                inside = np.all(lo >= 0, axis=1) & np.all(lo < np.asarray(self._gd, dtype=int), axis=1)
                lo, hi = lo[inside], hi[inside]
            if self._skip > 1:
                keep = np.all(lo % self._skip == 0, axis=1)
                lo, hi = lo[keep], hi[keep]
            self._list = list(zip(lo, hi))
        return self._list

    def __len__(self):
        return len(self._get())

    def __iter__(self):
        return iter(self._get())

    def __getitem__(self, n):
        return self._get()[n]


class TriangulatedIsosurfaces(Delta3DContour):
    """TriangulatedIsosurfaces(mins, maxes, delta, function, value, segment_endpoints, ...)
    (tetrahedral.py:89-101).  `function` may be a callable f(x, y, z) in world coordinates (sampled
    once, vectorised when it broadcasts) or a dense sample array / GPU tensor of shape
    grid_dimensions+1."""

    def __init__(self, mins, maxes, delta, function, value, segment_endpoints,
                 linear_interpolate=True, flatten=False, minimum_ratio=None, minimum_extent=None,
                 smooth=None, device=None):
        self.flatten = flatten
        self.smooth = smooth
        self.device = device
        if minimum_ratio is not None:
            self.minimum_ratio = minimum_ratio
        if minimum_extent is not None:
            self.minimum_extent = minimum_extent
        if callable(function):
            grid = grid_field.FunctionGrid(mins, maxes, delta, function)
        else:
            grid = grid_field.FunctionGrid.from_array(function, mins, delta)
        Delta3DContour.__init__(self, grid, value, segment_endpoints, linear_interpolate=linear_interpolate)


def _loop_points(points, loops, verts, mins=None, delta=None):
    "one (count, 3) float64 array per boundary loop: the rows of `points` its vertex indices name, mapped to grid * delta + mins"
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if mins is not None or delta is not None:
        d = np.ones(3) if delta is None else np.asarray(delta, dtype=np.float64)
        m = np.zeros(3) if mins is None else np.asarray(mins, dtype=np.float64)
        P = P * d + m if len(P) else P
    return [P[verts[int(r["first"]):int(r["first"]) + int(r["count"])]] for r in loops]


class LevelResult(tuple):
    """(value, points, triangles) of one level of MultiLevelIsosurfaces.levels(), with the vertex attributes of that level:
    vertex_normals() / vertex_curvature() / vertex_values(field).  They read the level's mesh on the device, so they work until the
    generator moves on to the next level."""

    def _bind(self, owner, index, post, delta, mins=None):
        self._owner, self._index, self._post, self._delta = owner, index, post, delta
        self._mins = (0.0, 0.0, 0.0) if mins is None else mins
        return self

    def _ctx(self):
        if self._owner._current != self._index:
            raise RuntimeError("level %d is no longer the current level of the context: ask for its attributes before advancing levels()" % self._index)
        return self._owner._ctx

    def vertex_normals(self, device=False):
        "(V,3) float64 unit normals in world coordinates, row i for points[i]"
        return self._ctx().level1_normals(self._post, self._delta, device)

    def vertex_curvature(self, device=False):
        "(V,4) float64 {mean, gauss, k1, k2} in world units, row i for points[i], signed like vertex_normals()"
        return self._ctx().level1_curvature(self._post, self._delta, device)

    def vertex_values(self, field, device=False):
        "(V,) float64: a second grid of the samples' shape at the vertices"
        return self._ctx().level1_sample(self._post, field, device)

    def components(self, device=False):
        "the level's components in world coordinates (GridContour3d.components); device=True: with the labels as device tensors"
        ctx = self._ctx()
        table = ctx.level1_components(self._mins, self._delta)
        return (table,) + tuple(ctx.level1_component_labels(device=True)) if device else table

    def component_labels(self, device=False):
        "(triangle labels in the order of the level's sorted triangle rows, vertex labels); device=True: tensors in device order"
        ctx = self._ctx()
        if device:
            return ctx.level1_component_labels(device=True)
        tl, vl = ctx.level1_component_labels()
        _pts, tris = ctx.download_level1(self._post)
        return tl[surface_geometry.row_order(tris)], vl

    def topology(self, device=False):
        "the topology of the level's components (GridContour3d.topology)"
        return self._ctx().level1_topology(device)

    def boundary_loops(self, device=False):
        "the boundary loops of the level's mesh (GridContour3d.boundary_loops), the points in world coordinates"
        ctx = self._ctx()
        if device:
            return ctx.level1_boundary_loops(device=True)
        loops, verts = ctx.level1_boundary_loops()
        return loops, verts, _loop_points(ctx.download_level1(self._post)[0], loops, verts, self._mins, self._delta)

    def keep_components(self, mask=None, largest=None, min_triangles=None, min_area=None, closed=None, genus=None, boundary_loops=None):
        """drop components of the level's mesh on the device (GridContour3d.keep_components, min_area in world units); the tuple's
        own points and triangles are the unfiltered ones: mesh() downloads the filtered mesh"""
        ctx = self._ctx()
        topo = ctx.level1_topology() if (genus is not None or boundary_loops is not None) else None
        keep = surface_geometry.select_components(ctx.level1_components(self._mins, self._delta), mask, largest, min_triangles, min_area, closed,
                                                  topo, genus, boundary_loops)
        counts = ctx.level1_keep_components(keep)
        self._post = dict(self._post, **counts)
        return counts

    def simplify(self, cell=None, target_triangles=None, by_component=True, clean=True, normals="auto"):
        """GridContour3d.simplify on the level's mesh (`cell` in voxels); the tuple's own points and triangles are the unsimplified
        ones: mesh() downloads the simplified mesh"""
        if (cell is None) == (target_triangles is None):
            raise ValueError("exactly one of cell and target_triangles is needed")
        ctx = self._ctx()
        if normals == "auto":
            normals = bool(self._post.get("carried_normals", True))
        corner = max(int(n) for n in self._owner.grid.grid_dimensions)
        counts = _simplify_on(ctx, cell, target_triangles, by_component, clean, bool(normals), corner, self)
        self._post = dict(self._post, carried_normals=bool(normals), **{k: counts[k] for k in ("n_vertices", "n_triangles", "n_components")})
        return counts

    def simplify_map(self, device=False):
        "GridContour3d.simplify_map for the level's mesh"
        return self._ctx().level1_simplify_map(getattr(self, "_simplify_n_old", 0), device)

    def clip(self, plane=None, box=None, field=None, scalars=None, value=0.0, keep="above", clean=True, normals="auto", mins=None, delta=None):
        """GridContour3d.clip on the level's mesh; plane and box in WORLD coordinates (the level's mins and delta, unless mins / delta
        are given).  The tuple's own points and triangles are the unclipped ones: mesh() downloads the clipped mesh"""
        mins = self._mins if mins is None else mins
        delta = self._delta if delta is None else delta
        spec = _clip_args(plane, box, field, scalars, keep, mins, delta)
        ctx = self._ctx()
        if normals == "auto":
            normals = bool(self._post.get("carried_normals", True))
        counts = _clip_on(ctx, spec, value, keep, clean, bool(normals))
        self._post = dict(self._post, carried_normals=bool(normals), **{k: counts[k] for k in ("n_vertices", "n_triangles", "n_components")})
        return counts

    def clip_map(self, device=False):
        "GridContour3d.clip_map for the level's mesh"
        return self._ctx().level1_clip_map(device)

    def clip_values(self, values):
        "GridContour3d.clip_values for the level's mesh"
        return _clip_values(values, self._ctx())

    def mesh(self):
        "(world points, sorted triangle rows) of the level's mesh as it stands on the device (after keep_components or simplify: that one)"
        ctx = self._ctx()
        pts, tris = ctx.download_level1(self._post)
        delta, mins = np.asarray(self._delta, dtype=np.float64), np.asarray(self._mins, dtype=np.float64)
        return (pts * delta + mins if len(pts) else np.zeros((0, 3))), surface_geometry.sort_rows(tris)


class MultiLevelIsosurfaces(object):
    """Several isovalues of ONE field (BASELINE.json config 5; the reference has this only in 2-D,
    contourist/multiple_2d_contour.py:17-75).  The dense samples are bound to the device once and ALL levels are
    marched in one call: one pass over the samples classifies every level (`cx_extract3d_levels`), then the
    vertex / triangle stages and the Level-1 post-pass run per level.  `levels()` yields (value, points, triangles)
    in ascending value order; every level equals what a TriangulatedIsosurfaces of that value returns."""

    def __init__(self, mins, maxes, delta, function, values, device=None, diagonal="cpython310"):
        self.values = sorted(float(v) for v in values)
        if callable(function):
            self.grid = grid_field.FunctionGrid(mins, maxes, delta, function)
        else:
            self.grid = grid_field.FunctionGrid.from_array(function, mins, delta)
        self.device = _DEFAULT_DEVICE[0] if device is None else int(device)
        self.flags = {"cpython310": _ffi.CX_DIAG_CPYTHON310, "canonical": _ffi.CX_DIAG_CANONICAL}[diagonal]
        self._ctx = _ffi.Context(self.device)
        self.counts = None
        self._current = None
        self._bound = False           # the context holds this object's samples (levels() binds them anew; spectrum() only if needed)

    @classmethod
    def at_quantiles(cls, mins, maxes, delta, function, q, **kw):
        """the levels at the q-quantiles (q in [0, 1]) of the field's own samples, NaN samples left out: exact order statistics
        taken on the device (levels.quantiles), no sort and no sample of the samples"""
        from . import levels as _levels
        made = cls(mins, maxes, delta, function, (), **kw)
        made.values = sorted(float(v) for v in _levels.quantiles(made.grid.dense_samples(), q, made.device))
        return made

    def _bind_grid(self, samples):
        shape = tuple(int(n) for n in samples.shape)
        ctx = self._ctx
        if grid_field._is_torch(samples):
            assert samples.is_cuda and samples.is_contiguous() and _ffi.native_dtype(samples.dtype), \
                "device samples must be a contiguous tensor on the GPU of a supported dtype (%s)" % ", ".join(_ffi.DTYPE_CODES)
            ctx.adopt_device_grid(samples.data_ptr(), shape, keepalive=samples, dtype=samples.dtype)
        else:
            ctx.upload_grid_native(samples)
        ctx.set_origin(0, 0, 0)
        ctx.set_reference_corner((0, 0, 0))
        self._bound = True

    def spectrum(self, values=None):
        """the size of the surface at every one of `values` (default: the object's own), without marching any: dict of four int64
        arrays in the order of `values` -- n_cells (whole cells the surface passes through), n_vertices, n_triangles (the march's
        n_border_voxels, n_vertices and n_triangles at that value wherever n_near is 0) and n_near.  One pass over the samples for
        all values; levels already marched stay as they are."""
        from . import levels as _levels
        if not self._bound:
            self._bind_grid(self.grid.dense_samples())
        return _levels.spectrum_of_context(self._ctx, self.values if values is None else values)

    def levels(self, clean=True, cap=None):
        """cap: None, or the faces of GridContour3d.cap_rim ("all", a mask, names) -- every level is then capped (side "above") after it is
        selected, exactly as a single capped extraction of that value"""
        cap_mask = None if cap is None else _ffi.cap_faces_mask(cap)
        samples = self.grid.dense_samples()
        corner = tuple(int(n) for n in self.grid.grid_dimensions)
        shape = tuple(int(n) for n in samples.shape)
        ctx = self._ctx
        if shape[2] < 4:          # rows shorter than 4 samples take the shape-agnostic kernel: one level at a time
            self._bound = False
            for n, v in enumerate(self.values):
                maker = GridContour3d(corner, samples, v, None, context=ctx)
                if cap_mask is not None:
                    maker.cap_rim(cap_mask)
                grid_points, triangles = maker.get_points_and_triangles(clean)
                self._current = n
                yield LevelResult((v, self.grid.from_grid_coordinates(grid_points) if len(grid_points) else np.zeros((0, 3)),
                                   triangles))._bind(self, n, maker._post, self.grid.delta, self.grid.mins)
            self._current = None
            return
        self._bind_grid(samples)
        self.counts = ctx.extract3d_levels(self.values, self.flags)
        for n, v in enumerate(self.values):
            ctx.select_level(n)
            if cap_mask is not None:
                ctx.cap3d(cap_mask, "above")
                post = dict(ctx.postprocess3d_capped(0 if clean else 1), capped=True, carried_normals=False)
            else:
                post = ctx.postprocess3d(0 if clean else 1)
            grid_points, triangles = ctx.download_level1(post)
            geometry = surface_geometry.SurfaceGeometry._from_device(grid_points, triangles, ctx)   # sorted rows, as the reference returns them
            points = self.grid.from_grid_coordinates(geometry.vertices) if len(grid_points) else np.zeros((0, 3))
            self._current = n
            yield LevelResult((v, points, geometry.oriented_triangles))._bind(self, n, post, self.grid.delta, self.grid.mins)
        self._current = None


def rim_crossing_segments(S, gd, v, shell=2):
    """the crossing lattice segments of find_contour_crossing_grid_segments (grid_field.py:64-84: from every lattice point
    0 <= p < grid_dimensions to its 2^d - 1 forward neighbours, strict sign change) that lie within `shell` lattice steps of
    the rim of the grid, IN THE REFERENCE'S ORDER (points in index order, last axis fastest; neighbours in the order of
    surrounding_vertices :52-62, first axis fastest).  Any dimension.  S: samples at the vertices 0 .. gd inclusive.
    None if no segment touches the rim itself."""
    gd = np.asarray(gd, dtype=int)
    d = len(gd)
    base = S[tuple(slice(0, int(n)) for n in gd)]
    near = np.zeros(tuple(gd), dtype=bool)        # lower end within the shell
    for a in range(d):
        sl = [slice(None)] * d
        sl[a] = slice(0, shell + 1)
        near[tuple(sl)] = True
        sl[a] = slice(max(int(gd[a]) - 1 - shell, 0), int(gd[a]))
        near[tuple(sl)] = True
    rows, touches = [], False
    for index in range(1, 2 ** d):
        o = np.array([(index >> a) & 1 for a in range(d)])          # first axis fastest (:58-61)
        nb = S[tuple(slice(int(o[a]), int(o[a]) + int(gd[a])) for a in range(d))]
        hit = np.argwhere(((base - v) * (nb - v) < 0) & near)
        if len(hit) == 0:
            continue
        upper = hit + o
        touches = touches or bool(np.any(hit == 0) or np.any(upper == gd))
        lin = np.ravel_multi_index(tuple(hit.T), tuple(int(n) for n in gd))
        rows.append(np.concatenate([lin[:, None], np.full((len(hit), 1), index), hit, upper], axis=1))
    if not rows or not touches:
        return None
    R = np.concatenate(rows, axis=0)
    R = R[np.lexsort((R[:, 1], R[:, 0]))]
    return [(r[2:2 + d].astype(int), r[2 + d:2 + 2 * d].astype(int)) for r in R]


def refined_crossing_points(feval, z, lo, hi):
    """contour_pair_interpolation (tetrahedral.py:471-512) with linear_interpolate == False, iterations = 5, for many crossing
    edges at once, any dimension.  feval(P (N,d) float64) -> f at the rows; lo, hi: (N,d) integer lattice points of the edges
    (the coordinates f expects).  -> (N,d) float64 points in those coordinates."""
    low_a, high_a = np.asarray(lo).astype(np.float64), np.asarray(hi).astype(np.float64)
    lo_f, hi_f = low_a.copy(), high_a.copy()
    flow, fhigh = feval(low_a), feval(high_a)
    swap = flow > fhigh                                                  # :478-480
    low_a[swap], high_a[swap] = hi_f[swap], lo_f[swap]
    flow, fhigh = np.where(swap, fhigh, flow), np.where(swap, flow, fhigh)
    crosses = (flow <= z) & (fhigh >= z)
    den = 1.0 * (fhigh - flow)
    flat = np.abs(den) <= 1e-8                                           # np.allclose(denominator, 0)
    ratio = np.where(flat, 0.5, (z - flow) / np.where(flat, 1.0, den))
    P = low_a + ratio[:, None] * (high_a - low_a)
    P[~crosses] = low_a[~crosses]                                        # ":509 temporary hack": interpolated = low_a
    active = crosses.copy()
    fint = np.full(len(P), z, dtype=np.float64)
    if active.any():
        fint[active] = feval(P[active])
    for _ in range(5):                                                   # iterations=5
        close_f = np.abs(fint - z) <= 1e-8 + 1e-5 * abs(z)
        close_p = np.all(np.abs(low_a - high_a) <= 1e-8 + 1e-5 * np.abs(high_a), axis=1)
        active = active & ~close_f & ~close_p
        if not active.any():
            break
        below = active & (fint < z)
        above = active & ~(fint < z)
        low_a[below], flow[below] = P[below], fint[below]
        high_a[above], fhigh[above] = P[above], fint[above]
        r = (z - flow[active]) * 1.0 / (fhigh[active] - flow[active])
        P[active] = low_a[active] + r[:, None] * (high_a[active] - low_a[active])
        fint[active] = feval(P[active])
    return P
