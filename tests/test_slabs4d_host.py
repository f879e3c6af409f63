"""Host logic of the 4-D slab path (a volume of more than GridContour4D.MAX_SAMPLES_PER_EXTRACTION samples, marched slab by slab
and assembled on the device): which volumes take it, how they are cut into slabs, and what it refuses -- all before any GPU work."""
import numpy as np
import pytest


def _gc(shape, **kw):
    from contourist_amd import pentatopes
    A = np.zeros(shape, dtype=np.float32)
    return pentatopes.GridContour4D(tuple(n - 1 for n in shape), A, 0.5, **kw)


def test_the_limit_and_the_slab_planes():
    from contourist_amd import pentatopes, tetrahedral
    G = pentatopes.GridContour4D
    assert G.MAX_SAMPLES_PER_EXTRACTION == 1 << 28
    assert G._slab_bounds is tetrahedral.GridContour3d._slab_bounds or G._slab_bounds(10, 4) == tetrahedral.GridContour3d._slab_bounds(10, 4)

    class Fake(object):
        MAX_SAMPLES_PER_EXTRACTION = 1 << 28
        shape = (136, 128, 128, 128)
    assert (136 * 128 ** 3) > (1 << 28)
    assert G._in_slabs(Fake()) and not G._in_slabs(type("S", (Fake,), {"shape": (128, 128, 128, 128)})())
    planes = G._slab_planes(Fake())
    assert (planes + 1) * 128 ** 3 <= (1 << 28) < (planes + 2) * 128 ** 3
    for n0 in (2, 3, 17, 136, 257):
        b = G._slab_bounds(n0, planes)
        assert b[0][0] == 0 and b[-1][1] == n0 and all(b[k][1] == b[k + 1][0] for k in range(len(b) - 1))
        # every slab with its halo plane (all but the last) fits one extraction
        assert all(((i1 - i0) + (1 if i1 < n0 else 0)) * 128 ** 3 <= (1 << 28) for (i0, i1) in b)
    # a 256^3 series of 32 steps: 2^29 samples, slabs of 127 planes + halo
    big = type("B", (Fake,), {"shape": (256, 256, 256, 32)})()
    assert G._in_slabs(big) and G._slab_planes(big) == 127 and G._slab_bounds(256, 127) == [(0, 127), (127, 254), (254, 256)]
    with pytest.raises(ValueError):
        G._slab_planes(type("W", (Fake,), {"shape": (4, 1024, 1024, 128)})())


def test_small_volumes_keep_the_single_extraction():
    m = _gc((6, 5, 5, 4))
    assert not m._in_slabs()
    m.MAX_SAMPLES_PER_EXTRACTION = 5 * 5 * 4 * 3
    assert m._in_slabs() and m._slab_planes() == 2
    assert m._slab_bounds(6, 2) == [(0, 2), (2, 4), (4, 6)]


@pytest.mark.parametrize("case", ["end_points", "voxel_range", "not_linear", "origin"])
def test_refusals_name_the_limit_before_any_gpu_work(case):
    kw = {"end_points": dict(segment_endpoints=[((1, 1, 1, 1), (2, 2, 2, 2))]),
          "voxel_range": dict(voxel_range=((1, 1, 1, 1), (4, 4, 4, 3))),
          "not_linear": dict(linear_interpolate=False, function=lambda i, j, k, l: i + j + k + l),
          "origin": dict(origin=(-1, -1, -1, -1))}[case]
    m = _gc((6, 5, 5, 4), **kw)
    m.MAX_SAMPLES_PER_EXTRACTION = 5 * 5 * 4 * 3
    with pytest.raises(NotImplementedError, match="marched in slabs"):
        m.find_tetrahedra()
    assert m._ctx is None                           # refused before a context (and the GPU) was touched


def test_march_has_no_single_extraction_of_a_slab_volume():
    m = _gc((6, 5, 5, 4))
    m.MAX_SAMPLES_PER_EXTRACTION = 5 * 5 * 4 * 3
    with pytest.raises(NotImplementedError, match="no single Level-0 extraction"):
        m.march()
    assert m._ctx is None


def test_a_plane_too_large_for_two_planes_and_a_halo():
    m = _gc((6, 5, 5, 4))
    m.MAX_SAMPLES_PER_EXTRACTION = 5 * 5 * 4 * 2        # room for two planes, not for two and a halo
    with pytest.raises(ValueError, match="no room"):
        m.find_tetrahedra()
    assert m._ctx is None


def test_a_callable_whose_surface_touches_the_rim_is_refused(monkeypatch):
    """search_for_endpoints sends such a field to the seeded rim path (end points, a rim of samples): outside the slab path"""
    from contourist_amd import pentatopes
    monkeypatch.setattr(pentatopes.GridContour4D, "MAX_SAMPLES_PER_EXTRACTION", 64)

    def f(x, y, z, t):
        return x + 0.5 * y - 0.25 * z + 0.1 * t         # a plane through the whole box: it reaches the rim
    S = pentatopes.MorphingIsoSurfaces([0.0] * 4, [1.0] * 4, [0.25] * 4, f, 1.0, None)
    S.search_for_endpoints()
    assert S.contour_maker.end_points is not None and len(S.contour_maker.end_points)
    with pytest.raises(NotImplementedError, match="marched in slabs"):
        S.collect_morph_triangles()
    assert S.contour_maker._ctx is None
