"""cx_grid_resample3d (csrc/cx_resample.hip) against its numpy restatement (tests/resample_ref.py), bit for bit, n_outside included:
shapes around the bricks of both kernels (the general one: 4 x 4 x 16 outputs, the 16 along the output axis that runs along input axis
2; the table kernel of axis-aligned maps: 2 x 2 x 64), the maps that reach each of them, the three boundary rules and both orders,
every sample type from the host and from a device tensor, misaligned device slices, a caller's output, NaN and infinite samples,
contourist_amd.volume, the end-to-end routes with no host copy, what a call leaves alone and what a bind resets, the error codes."""
import itertools
import os

import numpy as np
import pytest

import resample_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

# the last brick is partial along every axis whichever way the general kernel's 4 x 4 x 16 brick is turned (7 = 4 + 3 = 16 - 9,
# 81 = 5 x 16 + 1 = 20 x 4 + 1) and for the table kernel's 2 x 2 x 64 (7 = 3 x 2 + 1, 81 = 64 + 17)
STRADDLE_4x4x16_2x2x64 = (7, 7, 81)
# (input shape, output shapes): the last output axis 1, 63, 64, 65 and 131 long
SHAPES = [((2, 2, 2), [(3, 5, 1), (2, 3, 63)]), ((1, 8, 9), [(4, 2, 64)]), ((5, 4, 3), [(3, 3, 65)]),
          ((7, 6, 9), [(2, 2, 131), STRADDLE_4x4x16_2x2x64])]
EYE = np.eye(3)


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def field(shape, seed, dtype=np.float32):
    rng = np.random.RandomState(seed)
    if np.dtype(dtype).kind == "f":
        return (rng.standard_normal(shape) * 3.0).astype(dtype)
    info = np.iinfo(dtype)
    return rng.randint(info.min, info.max + 1, size=shape).astype(dtype)


def centred_zoom(f):
    d = np.ones(3) / np.asarray(f, dtype=np.float64)
    return lambda n, m: (np.diag(d), 0.5 * d - 0.5)


def permutation(perm, flip):
    def make(n, m):
        M = np.zeros((3, 3))
        for k in range(3):
            M[perm[k], k] = -1.0 if flip else 1.0
        return M, (np.asarray(n, dtype=np.float64) - 1.0 if flip else np.zeros(3))
    return make


def rotated(axis):
    return lambda n, m: R.about_centre(R.rotation(axis, 30.0), n, m)


TINY = EYE.copy()
TINY[2, 1] = 1e-9      # next to its diagonal twin: the coordinate of axis 2 now depends on two output indices
# (input shape, output shape) -> (matrix, offset)
MAPS = {
    "identity": lambda n, m: (EYE, np.zeros(3)),
    "integer_shift": lambda n, m: (EYE, np.array([1.0, -2.0, 3.0])),
    "half_sample_shift": lambda n, m: (EYE, np.array([0.5, -0.5, 0.5])),
    "zoom_2": centred_zoom(2.0),
    "zoom_half": centred_zoom(0.5),
    "zoom_third": centred_zoom(1.0 / 3.0),
    "zoom_per_axis": centred_zoom((2.0, 0.5, 1.0 / 3.0)),
    "zoom_inexact_steps": centred_zoom((0.7, 1.3, 2.3)),      # steps whose products with an index are rounded: a fused multiply-add would show
    "rotate_0": rotated(0), "rotate_1": rotated(1), "rotate_2": rotated(2),
    "shear_mostly_outside": lambda n, m: (np.array([[1.5, 0.7, 0.3], [-0.4, 1.2, 0.9], [0.8, -0.6, 1.7]]), np.array([-3.0, 2.0, -5.0])),
    "tiny_off_diagonal": lambda n, m: (TINY, np.array([0.25, 0.0, -0.25])),
    "tiny_off_diagonal_twin": lambda n, m: (EYE, np.array([0.25, 0.0, -0.25])),
    "broadcast_plane": lambda n, m: (np.diag([0.0, 1.0, 1.0]), np.array([0.5, 0.0, 0.0])),      # a row without an entry
}
for _p in itertools.permutations(range(3)):
    for _flip in (False, True):
        MAPS["permute_%d%d%d%s" % (_p + ("_flipped" if _flip else "",))] = permutation(_p, _flip)


def check(ctx, A, M, off, out_shape, order, mode, cval, samples=None, dtype=None):
    "the device result of host samples A (or of `samples`) == the restatement on A, byte for byte, and so is n_outside"
    want, want_outside = R.resample(A, M, off, out_shape, order, mode, cval, dtype=dtype)
    n_outside, got = ctx.resample_grid(M, off, out_shape, order, mode, cval, samples=A if samples is None else samples, download=True)
    assert n_outside == want_outside, (n_outside, want_outside)
    assert not (want.dtype.kind == "f" and np.isnan(want).any())
    assert R.same_bytes(got, want), (got.dtype, want.dtype, got.shape, want.shape)
    return got, n_outside


@pytest.mark.parametrize("name", sorted(MAPS))
def test_maps_shapes_modes_and_orders(ctx, name):
    outside = 0
    for in_shape, out_shapes in SHAPES:
        A = field(in_shape, 11)
        for out_shape in out_shapes:
            M, off = MAPS[name](in_shape, out_shape)
            for mode in R.MODES:
                for order in (0, 1):
                    outside += check(ctx, A, M, off, out_shape, order, mode, 1.5)[1]
    if name == "shear_mostly_outside":
        total = 6 * sum(int(np.prod(o)) for _, outs in SHAPES for o in outs)
        assert outside > total // 2


def test_both_kernels_on_many_bricks(ctx):
    "2^20 outputs, 4096 bricks: every XCD's run of the numbering, a rotation (general kernel) and a zoom (table kernel); twice: the same bytes"
    A = field((40, 50, 60), 12)
    out_shape = (64, 64, 256)
    for M, off in (R.about_centre(R.rotation((1.0, 1.0, 1.0), 30.0) * 0.3, A.shape, out_shape),
                   (np.diag([40.0 / 64, 50.0 / 64, 60.0 / 256]), np.array([-0.1, -0.2, -0.3]))):
        got, n_outside = check(ctx, A, M, off, out_shape, 1, "reflect", 0.0)
        ctx.resample_grid(EYE, np.zeros(3), (3, 3, 3), samples=field((3, 3, 3), 1), download=True)      # (the scratch is reused in between)
        again_outside, again = ctx.resample_grid(M, off, out_shape, 1, "reflect", 0.0, samples=A, download=True)
        assert again.tobytes() == got.tobytes() and again_outside == n_outside
        check(ctx, A.astype(np.float16), M, off, out_shape, 0, "constant", -2.0)


TYPE_MAPS = [(np.diag([2.0, 0.5, 1.25]), np.array([-0.5, 0.25, -1.0])),                                  # table kernel
             (R.rotation((1.0, 2.0, 3.0), 40.0) * 0.9, np.array([1.0, 2.0, -3.0]))]                      # general kernel


@pytest.mark.parametrize("name", ["float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16"])
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    shape, out_shape = (7, 9, 20), (6, 10, 70)
    if name == "bfloat16":
        t = torch.from_numpy(field(shape, 9)).cuda().to(torch.bfloat16)
        A = t.view(torch.int16).cpu().numpy().view(np.uint16)
        host, dtype, cval = (A, "bfloat16", shape), "bfloat16", 1.5
    else:
        A = field(shape, 9, np.dtype(name))
        if name.startswith(("int", "uint")):
            info = np.iinfo(A.dtype)
            A[0, 0, :2] = [info.min, info.max]
        t = torch.from_numpy(A).cuda()
        host, dtype, cval = A, None, (1.5 if A.dtype.kind == "f" else 3.0)
    torch.cuda.synchronize()
    for M, off in TYPE_MAPS:
        for order in (0, 1):
            for mode in ("reflect", "constant"):
                a, _ = check(ctx, A, M, off, out_shape, order, mode, cval, samples=host, dtype=dtype)
                b, _ = check(ctx, A, M, off, out_shape, order, mode, cval, samples=(t.data_ptr(), t.dtype, shape), dtype=dtype)
                assert a.tobytes() == b.tobytes()


def test_misaligned_device_slice_and_callers_output(ctx):
    import torch
    from contourist_amd import _ffi
    shape, out_shape = (5, 9, 21), (6, 7, 71)
    n, m = int(np.prod(shape)), int(np.prod(out_shape))
    torch_types = {"float32": torch.float32, "uint8": torch.uint8, "int8": torch.int8, "uint16": torch.int16, "int16": torch.int16,
                   "float16": torch.float16, "bfloat16": torch.bfloat16}
    for name in sorted(torch_types):
        if name == "bfloat16":
            flat_t = torch.from_numpy(field(n + 1, 30)).cuda().to(torch.bfloat16)
            flat = flat_t.view(torch.int16).cpu().numpy().view(np.uint16)
        else:
            flat = field(n + 1, 30, np.dtype(name))
            flat_t = torch.from_numpy(flat.view(np.int16) if name == "uint16" else flat).cuda()
        t = flat_t[1:]      # the input pointer is one element off its allocation
        assert t.data_ptr() % 16 != 0
        A = flat[1:].reshape(shape)
        for (M, off), order in itertools.product(TYPE_MAPS, (0, 1)):
            cval = 1.5 if name in ("float32", "float16", "bfloat16") else 3.0
            want, want_outside = R.resample(A, M, off, out_shape, order, "constant", cval, dtype=name if name == "bfloat16" else None)
            out = torch.full((m + 2,), 7, dtype=torch_types[name] if order == 0 else torch.float32, device="cuda")
            guard = out[:1].cpu().view(torch.uint8).numpy().tobytes()      # the bytes of one element of the fill
            torch.cuda.synchronize()
            n_outside, ptr = ctx.resample_grid(M, off, out_shape, order, "constant", cval, samples=(t.data_ptr(), name, shape), out=out[1:].data_ptr())
            torch.cuda.synchronize()
            assert n_outside == want_outside and ptr == out[1:].data_ptr()
            raw, size = out.cpu().view(torch.uint8).numpy().tobytes(), want.dtype.itemsize
            assert len(guard) == size and raw[:size] == guard and raw[-size:] == guard      # nothing written around the result
            assert raw[size:-size] == want.tobytes(), (name, order)
            with pytest.raises(_ffi.CxError) as e:      # with an output of the caller's the context holds no result
                ctx.resample_result()
            assert e.value.code == _ffi.CX_ERR_STATE


def test_nan_and_infinite_samples(ctx):
    A = field((9, 12, 30), 13)
    A[2, 3, 4], A[5, 6, 20], A[7, 1, 13], A[5, 6, 21] = np.nan, np.inf, -np.inf, -np.inf      # (+inf beside -inf: inf - inf in the blend)
    seen_inf = False
    for M, off in TYPE_MAPS + [(EYE, np.zeros(3))]:
        for mode in R.MODES:
            want, want_outside = R.resample(A, M, off, (10, 12, 70), 1, mode, 1.5)
            n_outside, got = ctx.resample_grid(M, off, (10, 12, 70), 1, mode, 1.5, samples=A, download=True)
            assert np.isnan(want).any() and np.isfinite(want).any()
            seen_inf = seen_inf or bool(np.isinf(want).any())
            assert n_outside == want_outside and R.same_bits_nan(got, want)
    assert seen_inf
    # the identity reproduces them (t == 0: the high corner does not enter), the NaN's payload included
    _, got = ctx.resample_grid(EYE, np.zeros(3), A.shape, 1, "nearest", samples=A, download=True)
    assert got.tobytes() == A.tobytes()
    _, got = ctx.resample_grid(EYE, np.zeros(3), A.shape, 0, "nearest", samples=A, download=True)
    assert got.tobytes() == A.tobytes()


def test_volume_module(ctx):
    import torch
    from contourist_amd import volume
    A = field((12, 17, 33), 15)
    U = field((12, 17, 33), 16, np.uint8)
    rot = R.about_centre(R.rotation((0.0, 1.0, 1.0), 30.0), A.shape, (10, 20, 40))
    for S in (A, U):
        t = torch.from_numpy(S).cuda()
        for order in (0, 1):
            want, want_outside = R.resample(S, rot[0], rot[1], (10, 20, 40), order, "reflect")
            got, n_outside = volume.resample(S, rot[0], rot[1], (10, 20, 40), order, "reflect", return_outside=True)
            assert R.same_bytes(got, want) and n_outside == want_outside
            got_t = volume.resample(t, rot[0], rot[1], (10, 20, 40), order, "reflect")
            assert got_t.is_cuda and got_t.dtype == (t.dtype if order == 0 else torch.float32) and R.same_bytes(got_t.cpu().numpy(), want)
            # a vector is a diagonal; no output shape: the samples' own
            assert R.same_bytes(volume.resample(S, [1.0, 0.5, 2.0], 0.25, order=order), R.resample(S, np.diag([1.0, 0.5, 2.0]), [0.25] * 3, S.shape, order)[0])
            for factor, align in ((2.0, "centers"), (0.5, "centers"), ((1.0, 1.5, 1.0 / 3.0), "corners")):
                diag, off, out = volume.zoom_map(S.shape, factor, align)
                want = R.resample(S, np.diag(diag), off, out, order, "nearest")[0]
                assert R.same_bytes(volume.zoom(S, factor, order, align=align), want)
                assert R.same_bytes(volume.zoom(t, factor, order, align=align).cpu().numpy(), want)
    z = volume.zoom(A, 2.0, align="corners")
    assert z.shape == (24, 34, 66) and all(z[c].tobytes() == A[c].tobytes() for c in itertools.product((0, -1), repeat=3))
    # regrid: from a coarser, shifted lattice, with and without a rotation
    args = ([-1.0, 0.5, 2.0], [0.5, 0.25, 1.25], (14, 11, 30), [-1.3, 0.9, 2.6], [0.3, 0.2, 1.0])
    for rotation in (None, R.rotation(2, 15.0)):
        got, n_outside, M, off = volume.regrid(A, *args, rotation=rotation, return_map=True, return_outside=True)
        want, want_outside = R.resample(A, M, off, (14, 11, 30), 1, "constant", 0.0)
        assert R.same_bytes(got, want) and n_outside == want_outside and 0 < n_outside < want.size
        assert R.same_bytes(volume.regrid(torch.from_numpy(A).cuda(), *args, rotation=rotation).cpu().numpy(), want)
        assert R.same_bytes(volume.regrid(U, *args, rotation=rotation, order=0, cval=7), R.resample(U, M, off, (14, 11, 30), 0, "constant", 7)[0])
    # reslice: one oblique plane
    origin, u, v = [2.0, 1.0, 3.0], [0.3, 0.5, 0.1], [0.1, -0.2, 0.9]
    image, n_outside = volume.reslice(A, origin, u, v, (20, 37), return_outside=True)
    Mr = np.zeros((3, 3))
    Mr[:, 1], Mr[:, 2] = u, v
    want, want_outside = R.resample(A, Mr, origin, (1, 20, 37), 1, "constant", 0.0)
    assert image.shape == (20, 37) and R.same_bytes(image, want[0]) and n_outside == want_outside
    assert R.same_bytes(volume.reslice(torch.from_numpy(U).cuda(), origin, u, v, (20, 37), order=0).cpu().numpy(), R.resample(U, Mr, origin, (1, 20, 37), 0, "constant", 0)[0][0])
    # two dimensions and one
    B = A[3]
    M2 = np.array([[0.8, 0.3], [-0.2, 1.1]])
    M3 = np.eye(3)
    M3[1:, 1:] = M2
    assert R.same_bytes(volume.resample(B, M2, [1.0, -0.5], (9, 40)), R.resample(B[None], M3, [0.0, 1.0, -0.5], (1, 9, 40))[0][0])
    assert R.same_bytes(volume.zoom(B[5], 3.0), R.resample(B[5][None, None], np.diag([1.0, 1.0, 1.0 / 3.0]), [0.0, 0.0, 0.5 * (1.0 / 3.0) - 0.5], (1, 1, 99))[0][0, 0])
    assert R.same_bytes(volume.zoom(torch.from_numpy(B).cuda(), (0.5, 2.0)).cpu().numpy(),
                        R.resample(B[None], np.diag([1.0, 2.0, 0.5]), [0.0, 0.5, -0.25], (1, 8, 66))[0][0])
    # float64 samples are rounded to float32 first
    assert R.same_bytes(volume.zoom(A.astype(np.float64) + 1e-12, 0.5), R.resample((A.astype(np.float64) + 1e-12).astype(np.float32), np.diag([2.0] * 3), [0.5] * 3, (6, 8, 16))[0])


def _mesh(c, value):
    from contourist_amd import _ffi
    counts = c.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
    return counts, c.download_level0_records(counts)


def _same_mesh(a, b):
    (c0, m0), (c1, m1) = a, b
    return c0 == c1 and np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1].view(np.uint32), m1[1].view(np.uint32)) and np.array_equal(m0[2], m1[2])


def test_upload_resample_bind_march():
    """a uint8 volume is uploaded, doubled in resolution and marched with no copy of the resampled volume on the host: the mesh is that
    of the restatement's array uploaded as float32"""
    from contourist_amd import _ffi, volume
    A = np.load(os.path.join(GOLDEN_DIR, "noise32_v0.npz"))["A"]
    lo, hi = float(A.min()), float(A.max())
    U = np.clip(np.rint((A - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)
    diag, off, out = volume.zoom_map(U.shape, 2.0)
    want, want_outside = R.resample(U, np.diag(diag), off, out, 1, "nearest")
    c, fresh = _ffi.Context(), _ffi.Context()
    try:
        c.upload_grid_native(U)
        before = _ffi.device_bytes(c.handle)[0]
        n_outside, ptr = c.resample_grid(np.diag(diag), off, out)      # the bound grid in, the context's own buffer out
        assert n_outside == want_outside and c.resample_result() == (out, ptr, "float32", n_outside)
        c.bind_resampled()
        assert c.shape == out and c.grid_info() == dict(dtype="float32", device_bytes=want.size * 4)
        # the uint8 grid went; the result, the table and the count stay: nothing the size of a second copy
        assert _ffi.device_bytes(c.handle)[0] - before <= want.size * 4 - U.size + (1 << 16)
        fresh.upload_grid(want)
        got, ref = _mesh(c, 127.3), _mesh(fresh, 127.3)
        assert _same_mesh(got, ref) and got[0]["n_triangles"] > 1000
    finally:
        c.close()
        fresh.close()


def test_order_0_mask_bound_as_uint8_feeds_distance_and_label():
    import distance_ref
    import label_ref
    from contourist_amd import _ffi, volume
    rng = np.random.RandomState(5)
    mask = (rng.uniform(size=(9, 10, 20)) < 0.35).astype(np.uint8)
    diag, off, out = volume.zoom_map(mask.shape, 2.0)
    want = R.resample(mask, np.diag(diag), off, out, 0, "nearest")[0]
    assert want.dtype == np.uint8 and 0 < want.sum() < want.size
    c = _ffi.Context()
    try:
        _, ptr = c.resample_grid(np.diag(diag), off, out, 0, samples=mask)
        assert c.resample_result()[2] == "uint8"
        # the pending pointer is a legal input of the other grid calls, and of this one
        assert c.label_grid(0.5, "high", 1, samples=(ptr, "uint8", out))[0] == label_ref.label(want, 0.5, "high", 1)[1]
        _, smooth = c.filter_grid([(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3, samples=(ptr, "uint8", out), download=True)
        import filter_ref
        assert smooth.tobytes() == filter_ref.filter3d(want, [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3).tobytes()
        c.bind_resampled()
        assert c.shape == out and c.grid_info() == dict(dtype="uint8", device_bytes=want.size)
        n_sites, dist = c.distance_grid(0.5, "below", "float32", download=True)
        assert n_sites == int(want.sum()) and dist.tobytes() == distance_ref.distance(want, 0.5, "below").tobytes()
        k, labels = c.label_grid(0.5, "high", 2, download=True)
        ref_labels, ref_k = label_ref.label(want, 0.5, "high", 2)
        assert k == ref_k and np.array_equal(labels, ref_labels)
        # the result of a call as the input of the next one
        _, ptr = c.resample_grid(np.diag([0.5] * 3), [0.0] * 3, out, 0)
        n2, twice = c.resample_grid(EYE, [0.0] * 3, out, 1, samples=(ptr, "uint8", out), download=True)
        assert twice.tobytes() == R.resample(R.resample(want, np.diag([0.5] * 3), [0.0] * 3, out, 0)[0], EYE, [0.0] * 3, out, 1)[0].tobytes()
    finally:
        c.close()


def test_regrid_makes_a_second_volume_legal_beside_the_marched_one():
    """a second volume on a coarser, shifted lattice is put on the marched grid's lattice on the device; vertex_values(field) and
    clip(field=...) take it and equal the same calls on the restatement's array"""
    import torch
    from contourist_amd import tetrahedral, volume
    A = np.load(os.path.join(GOLDEN_DIR, "noise32_v0.npz"))["A"].astype(np.float32)
    value = float(np.median(A))
    idx = np.meshgrid(*[np.arange(14, dtype=np.float64)] * 3, indexing="ij")
    B = (np.sin(0.4 * idx[0]) * 3.0 + 0.5 * idx[1] - 0.25 * idx[2]).astype(np.float32)      # 14^3 samples, steps of 2.5, from -1.25
    args = ([-1.25] * 3, 2.5, A.shape, [0.0] * 3, 1.0)
    field_t, n_outside, M, off = volume.regrid(torch.from_numpy(B).cuda(), *args, mode="nearest", return_map=True, return_outside=True)
    want, want_outside = R.resample(B, M, off, A.shape, 1, "nearest")
    assert field_t.is_cuda and tuple(field_t.shape) == A.shape and n_outside == want_outside == 0
    corner = tuple(n - 1 for n in A.shape)
    m = tetrahedral.GridContour3d(corner, A, value)
    m.get_points_and_triangles()
    s_dev, s_ref = m.vertex_values(field_t), m.vertex_values(want)
    assert len(s_ref) > 1000 and s_dev.tobytes() == s_ref.tobytes()
    threshold = float(np.median(s_ref))
    ctx = m.context()
    meshes = []
    for f in (field_t, want):
        m._post = None
        m._ensure_post(True)
        counts = m.clip(field=f, value=threshold, clean=False, normals=False)
        p, t = ctx.download_level1(m._post)
        meshes.append((counts, p.tobytes(), t.tobytes()))
    assert meshes[0] == meshes[1] and meshes[0][0]["n_cut_vertices"] > 0


def test_a_call_leaves_the_state_and_binding_resets_it():
    from contourist_amd import _ffi
    A = field((12, 13, 70), 19)
    M, off = R.about_centre(R.rotation(1, 30.0), A.shape, A.shape)
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)                                                # the other three pending results
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        n_outside, rptr = c.resample_grid(M, off, A.shape)                        # of the bound grid, into the context
        c.resample_grid(EYE, [0.0] * 3, (5, 6, 7), samples=field((5, 6, 7), 1), download=True)      # of other samples
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts               # the grid is the one uploaded
        levels = c.extract3d_levels([-0.4, 0.1, 0.6], _ffi.CX_DIAG_CPYTHON310)
        c.select_level(1)
        sel = c.download_level0_records(levels[1])
        n_outside, rptr = c.resample_grid(M, off, A.shape)
        assert c.counts() == levels[1]
        assert all(np.array_equal(a, b) for a, b in zip(sel, c.download_level0_records(levels[1])))
        c.select_level(2)
        assert c.counts() == levels[2]
        p = c.postprocess3d()
        # the four pending slots are independent
        assert c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k)
        filt = c.filter_grid(axes)
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)
        assert c.resample_result() == (A.shape, rptr, "float32", n_outside)
        # bind: as after an upload; the other three results stay
        c.bind_resampled()
        for gone in (c.counts, lambda: c.select_level(0), lambda: c.download_level1(p), c.resample_result, c.bind_resampled):
            with pytest.raises(_ffi.CxError) as e:
                gone()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert c.filter_result() == filt and c.distance_result() == dist and c.label_result() == (A.shape, lptr, "high", 2, k)
        assert c.shape == A.shape and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        again = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        fresh = _ffi.Context()
        try:
            fresh.upload_grid(R.resample(A, M, off, A.shape, 1)[0])
            assert fresh.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == again
        finally:
            fresh.close()
        # the bound grid resampled again, and bound again: the grid owned before is released
        live = _ffi.device_bytes(c.handle)[0]
        c.resample_grid(M, off, A.shape)
        c.bind_resampled()
        assert _ffi.device_bytes(c.handle)[0] == live
        # a result with an axis of length 1 is refused and stays pending
        n_outside, rptr = c.resample_grid(EYE, [0.0] * 3, (1, 13, 70))
        with pytest.raises(_ffi.CxError) as e:
            c.bind_resampled()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.resample_result() == ((1, 13, 70), rptr, "float32", 0) and c.shape == A.shape
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import torch
    from contourist_amd import _ffi
    A = field((4, 5, 6), 21)

    def code(M=EYE, off=(0.0, 0.0, 0.0), out_shape=(4, 5, 6), order=1, mode="nearest", cval=0.0, samples=A, **kw):
        with pytest.raises(_ffi.CxError) as e:
            ctx.resample_grid(M, off, out_shape, order, mode, cval, samples=samples, **kw)
        return e.value.code

    fresh = _ffi.Context()
    try:
        for call in (lambda: fresh.resample_grid(EYE, [0.0] * 3, (4, 5, 6)), fresh.resample_result, fresh.bind_resampled):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
    finally:
        fresh.close()
    for order in (-1, 2, 3):
        assert code(order=order) == _ffi.CX_ERR_INVALID
    _ffi.FILTER_MODES["wrap"] = 3
    try:
        assert code(mode="wrap") == _ffi.CX_ERR_INVALID
    finally:
        del _ffi.FILTER_MODES["wrap"]
    for cval in (float("nan"), float("inf"), -float("inf")):
        for order in (0, 1):
            assert code(cval=cval, order=order) == _ffi.CX_ERR_INVALID
            assert code(cval=cval, order=order, mode="constant") == _ffi.CX_ERR_INVALID
    for bad in (float("nan"), float("inf"), -float("inf"), 2.0 ** 20 + 1.0, -(2.0 ** 20) - 1.0):
        for at in range(9):
            M = EYE.copy()
            M.reshape(-1)[at] = bad
            assert code(M=M) == _ffi.CX_ERR_INVALID
        for at in range(3):
            off = [0.0] * 3
            off[at] = bad
            assert code(off=off) == _ffi.CX_ERR_INVALID
    ctx.resample_grid(EYE * 2.0 ** 20, [-(2.0 ** 20)] * 3, (2, 2, 2), samples=A)      # the bound itself is legal
    for out_shape in ((0, 5, 6), (4, -1, 6), (1 << 16, 1 << 16, 1), (1 << 11, 1 << 11, (1 << 9) + 1)):
        assert code(out_shape=out_shape) == _ffi.CX_ERR_INVALID
    # order 0: cval must be a value of the sample type
    for dtype, cval in ((np.uint8, 1.5), (np.uint8, -1.0), (np.uint8, 256.0), (np.int8, 128.0), (np.uint16, 65536.0), (np.int16, -32769.0),
                        (np.float16, 1.0 + 2.0 ** -11), (np.float16, 65536.0), (np.float32, 0.1)):
        S = np.zeros((2, 3, 4), dtype=dtype)
        assert code(samples=S, out_shape=(2, 3, 4), order=0, cval=cval) == _ffi.CX_ERR_INVALID, (dtype, cval)
        ctx.resample_grid(EYE, [0.0] * 3, (2, 3, 4), 1, "constant", cval, samples=S)      # (order 1 rounds it to float32)
    assert code(samples=(np.zeros(24, dtype=np.uint16), "bfloat16", (2, 3, 4)), out_shape=(2, 3, 4), order=0, cval=1.0 + 2.0 ** -8) == _ffi.CX_ERR_INVALID
    for dtype, cval in ((np.uint8, 255.0), (np.int8, -128.0), (np.float16, 65504.0), (np.float32, 0.5)):
        ctx.resample_grid(EYE, [0.0] * 3, (2, 3, 4), 0, "constant", cval, samples=np.zeros((2, 3, 4), dtype=dtype))
    t = torch.from_numpy(A).cuda()
    torch.cuda.synchronize()
    call = ctx.lib.cx_grid_resample3d
    mat, off, m = np.ascontiguousarray(EYE), np.zeros(3), np.asarray([4, 5, 6], dtype=np.int64)
    ok = (mat.ctypes.data, off.ctypes.data, m.ctypes.data, 1, 0, 0.0, None, None, None)
    for dtype in (7, -1):
        assert call(ctx.handle, t.data_ptr(), dtype, 1, 4, 5, 6, *ok) == _ffi.CX_ERR_INVALID
    for shape in ((0, 5, 6), (4, -1, 6), (1 << 16, 1 << 16, 1)):      # an empty axis, and more than 2^31 samples
        assert call(ctx.handle, t.data_ptr(), 0, 1, shape[0], shape[1], shape[2], *ok) == _ffi.CX_ERR_INVALID
    assert call(None, t.data_ptr(), 0, 1, 4, 5, 6, *ok) == _ffi.CX_ERR_INVALID
    for missing in range(3):
        args = list(ok)
        args[missing] = None
        assert call(ctx.handle, t.data_ptr(), 0, 1, 4, 5, 6, *args) == _ffi.CX_ERR_INVALID
    # an output that overlaps the input: the same memory, its last sample, the sample in front of it
    big = torch.zeros(3 * A.size, dtype=torch.float32, device="cuda")
    inner = big[A.size:2 * A.size]
    inner.copy_(t.reshape(-1))
    torch.cuda.synchronize()
    src = (inner.data_ptr(), inner.dtype, A.shape)
    assert code(samples=src, out=inner.data_ptr()) == _ffi.CX_ERR_INVALID
    assert code(samples=src, out=inner.data_ptr() + 4 * (A.size - 1)) == _ffi.CX_ERR_INVALID
    assert code(samples=src, out=big.data_ptr() + 4) == _ffi.CX_ERR_INVALID
    # next to it is fine
    M, o = R.about_centre(R.rotation(0, 30.0), A.shape, A.shape)
    ctx.resample_grid(M, o, A.shape, samples=src, out=big.data_ptr())
    ctx.synchronize()
    assert big[:A.size].cpu().numpy().reshape(A.shape).tobytes() == R.resample(A, M, o, A.shape, 1)[0].tobytes()


def test_a_pointer_into_the_pending_result():
    "planes 1 to 5 of the pending result as the samples of the next call, whose result the context keeps again: both kernels"
    from contourist_amd import _ffi
    A = field((6, 9, 70), 41)
    part = (5, 9, 70)
    for M, off in TYPE_MAPS:
        first = R.resample(A, M, off, A.shape, 1, "reflect", 0.0)[0]
        want, want_outside = R.resample(first[1:], M, off, part, 1, "reflect", 0.0)
        assert want_outside > 0
        c = _ffi.Context()
        try:
            _, ptr = c.resample_grid(M, off, A.shape, 1, "reflect", 0.0, samples=A)
            n_outside, got = c.resample_grid(M, off, part, 1, "reflect", 0.0, samples=(ptr + 9 * 70 * 4, "float32", part), download=True)
            assert n_outside == want_outside and R.same_bytes(got, want)
            assert c.resample_result()[::2] == (part, "float32")
        finally:
            c.close()
