"""cx_grid_label3d (csrc/cx_label.hip) against its numpy restatement (tests/label_ref.py), exactly: labels, K, every field of the records,
masks and their counts.  Shapes around the kernels' tiles (a wave owns a row and walks it in tiles of 64 columns), both sides, three
connectivities, random densities down to each connectivity's percolation threshold, and the patterns where labelling goes wrong: rows
and planes that must not wrap, contacts by face, edge and corner across tile boundaries, a numbering that differs from the order of
discovery, combs, a snake, checkerboards, nested shells.  Every sample type from the host and from a device tensor, the low rule,
misaligned slices and a caller's output with guards, contourist_amd.volume, the end-to-end routes label -> keep the largest -> bind ->
march and fill_holes -> signed distance -> bind -> march, what a call leaves alone and what a bind resets, and the error codes."""
import os

import numpy as np
import pytest

import distance_ref as D
import label_ref as R
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

STRADDLE = (37, 33, 259)      # 4 x 64 + 3 columns, rows and planes that are no multiple of a workgroup's four waves
PERCOLATION = {1: 0.31, 2: 0.14, 3: 0.1}      # site percolation thresholds of the cubic lattice with 6, 18, 26 neighbours (rounded)
DENSITIES = [0.5, 0.31, 0.14, 0.1, 0.03]
FIELDS = [f for f in R.RECORD_DTYPE.names]


@pytest.fixture(scope="module")
def ctx():
    from contourist_amd import _ffi
    c = _ffi.Context()
    yield c
    c.close()


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def same_records(got, want):
    assert len(got) == len(want)
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (f, got[f][:4], want[f][:4])


def keep_pattern(k):
    "K + 1 flags with both values among the labels and the unlabelled samples kept: 1 0 1 1 0 1 1 0 ..."
    return (np.arange(k + 1) % 3 != 1).astype(np.uint8)


def check(ctx, A, value, sides=R.SIDES, connectivities=(1, 2, 3), samples=None, expect_k=None):
    """labels, K, records and a mask of the device == the restatement, for host samples A (or `samples`, whose values are A's)"""
    from contourist_amd import _ffi
    src = A if samples is None else samples
    for side in sides:
        for c in connectivities:
            want, k = R.label(A, value, side, c)
            got_k, got = ctx.label_grid(value, side, c, samples=src, download=True)
            assert got_k == k, (side, c, got_k, k)
            if expect_k is not None:
                assert k == expect_k[c], (side, c, k)
            same(got, want)
            shape, ptr, got_side, got_c, kk = ctx.label_result()
            assert (shape, got_side, got_c, kk) == (A.shape, side, c, k) and ptr
            rec = ctx.label_measures()
            assert rec.dtype == _ffi.LABEL_COMPONENT_DTYPE == R.RECORD_DTYPE
            same_records(rec, R.records(want, k))
            for keep in (keep_pattern(k), 1 - keep_pattern(k)):
                n, mask = ctx.label_select(keep, download=True)
                want_mask, want_n = R.select(want, keep)
                assert n == want_n
                same(mask, want_mask)


def uniform(shape, seed):
    return np.random.RandomState(seed).uniform(size=shape).astype(np.float32)


SMALL = [(1, 1, 1), (2, 2, 2), (1, 8, 9), (5, 4, 3), (3, 5, 63), (3, 5, 64), (2, 6, 65), (2, 3, 131)]
CASES = [(shape, density, (1, 2, 3)) for shape in SMALL for density in DENSITIES]
for _c in (1, 2, 3):      # on the large shape: each connectivity at its own threshold, and the two ends
    CASES += [(STRADDLE, density, (_c,)) for density in (PERCOLATION[_c], 0.5, 0.03)]


@pytest.mark.parametrize("shape,density,connectivities", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_random_masks(ctx, shape, density, connectivities):
    "both sides: the labelled samples have this density"
    A = uniform(shape, 41)
    check(ctx, A, 1.0 - density, sides=("high",), connectivities=connectivities)
    check(ctx, A, density, sides=("low",), connectivities=connectivities)


def test_rows_and_planes_do_not_wrap(ctx):
    for a, b in ((((1, 1, 69), (1, 2, 0))), ((0, 3, 69), (1, 0, 0)), ((1, 3, 69), (2, 0, 0))):
        A = np.zeros((3, 4, 70), dtype=np.float32)
        A[a], A[b] = 1.0, 1.0
        check(ctx, A, 0.5, sides=("high",), expect_k={1: 2, 2: 2, 3: 2})
    A = np.zeros((2, 4, 64), dtype=np.uint8)      # the row ends where the tile ends
    A[0, 1, 63], A[0, 2, 0], A[0, 3, 63], A[1, 0, 0] = 1, 1, 1, 1
    check(ctx, A, 0.5, sides=("high",), expect_k={1: 4, 2: 4, 3: 4})


def test_contacts_by_face_edge_and_corner(ctx):
    "pairs of samples across the tile boundaries 63|64 and 127|128, across rows and across planes: K by construction"
    face, edge, corner = {1: 1, 2: 1, 3: 1}, {1: 2, 2: 1, 3: 1}, {1: 2, 2: 2, 3: 1}
    pairs = [
        ((1, 1, 63), (1, 1, 64), face), ((1, 1, 127), (1, 1, 128), face), ((1, 1, 63), (1, 2, 63), face), ((0, 1, 64), (1, 1, 64), face),
        ((1, 1, 63), (1, 2, 64), edge), ((1, 1, 64), (1, 2, 63), edge), ((1, 1, 127), (1, 2, 128), edge), ((1, 2, 127), (1, 1, 128), edge),
        ((0, 1, 63), (1, 1, 64), edge), ((0, 1, 128), (1, 1, 127), edge), ((0, 1, 5), (1, 2, 5), edge), ((0, 2, 64), (1, 1, 64), edge),
        ((0, 1, 63), (1, 2, 64), corner), ((0, 1, 64), (1, 2, 63), corner), ((0, 2, 127), (1, 1, 128), corner), ((0, 2, 128), (1, 1, 127), corner),
        ((0, 0, 0), (1, 1, 1), corner), ((1, 2, 129), (2, 3, 130), corner),
    ]
    for a, b, expect in pairs:
        A = np.zeros((3, 4, 131), dtype=np.uint8)
        A[a], A[b] = 1, 1
        check(ctx, A, 0.5, sides=("high",), expect_k=expect)
        # the same contact between two runs that reach over the tile boundaries, and with the rest of the array as the other side
        B = np.zeros((3, 4, 131), dtype=np.uint8)
        if a[2] <= b[2]:
            B[a[0], a[1], :a[2] + 1], B[b[0], b[1], b[2]:] = 1, 1
        else:
            B[a[0], a[1], a[2]:], B[b[0], b[1], :b[2] + 1] = 1, 1
        check(ctx, B, 0.5, sides=("high",), expect_k=expect if a[:2] != b[:2] else None)
        check(ctx, B, 0.5, sides=("low",))


def test_numbering_is_not_the_order_of_discovery(ctx):
    "a U whose arms join only in the last row of the last plane, and a dot between the arms: the U is 1, the dot is 2"
    A = np.zeros((3, 4, 70), dtype=np.float32)
    A[:, :, 5], A[:, :, 50], A[2, 3, 5:51], A[0, 0, 20] = 1, 1, 1, 1
    check(ctx, A, 0.5, sides=("high",), expect_k={1: 2, 2: 2, 3: 2})
    for c in (1, 2, 3):
        _, got = ctx.label_grid(0.5, "high", c, samples=A, download=True)
        assert got[0, 0, 5] == 1 and got[0, 0, 50] == 1 and got[0, 0, 20] == 2


def test_combs(ctx):
    shape = (9, 10, 70)
    for spine in (69, 0):      # teeth along axis 2 on every other row of every other plane, joined at one end
        A = np.zeros(shape, dtype=np.uint8)
        A[::2, ::2, :] = 1
        A[::2, :, spine] = 1
        check(ctx, A, 0.5, expect_k=None)
        assert R.label(A, 0.5, "high", 1)[1] == 5
    A = np.zeros(shape, dtype=np.uint8)      # teeth along axis 0, joined in the last plane
    A[:, ::2, ::2] = 1
    A[8, :, :] = 1
    check(ctx, A, 0.5)
    assert R.label(A, 0.5, "high", 1)[1] == 1


def test_a_snake(ctx):
    "long chains of unions: one path through the whole array, the first sample of which is at one end of it"
    shape = (9, 10, 70)
    A = np.zeros(shape, dtype=np.uint8)
    col = 0
    for i in range(0, 9, 2):
        rows = list(range(0, 10, 2)) if (i // 2) % 2 == 0 else list(range(8, -1, -2))
        for n, j in enumerate(rows):
            A[i, j, :] = 1
            col = 69 - col      # the row is walked to its other end
            if n + 1 < len(rows):
                A[i, (j + rows[n + 1]) // 2, col] = 1
        if i + 2 < 9:
            A[i + 1, rows[-1], col] = 1
    assert R.label(A, 0.5, "high", 1)[1] == 1 and R.label(A, 0.5, "low", 1)[1] == 1
    check(ctx, A, 0.5)
    # the same path cut once in the middle: two components whichever way the unions ran
    A[4, 4, 35] = 0
    check(ctx, A, 0.5, sides=("high",), connectivities=(1,), expect_k={1: 2})


def test_checkerboards(ctx):
    i, j, k = np.meshgrid(np.arange(37), np.arange(33), np.arange(259), indexing="ij")
    A = ((i + j + k + 1) % 2).astype(np.uint8)      # the corner sample is set
    # every sample its own component: K crosses many blocks of the scan, and the labels ascend with the linear index
    n, got = ctx.label_grid(0.5, "high", 1, samples=A, download=True)
    assert n == int(A.sum()) == 158120
    assert np.array_equal(got[A == 1], np.arange(1, n + 1, dtype=np.int32)) and not got[A == 0].any()
    rec = ctx.label_measures()
    assert np.array_equal(rec["first"], np.flatnonzero(A.reshape(-1))) and np.all(rec["voxels"] == 1)
    assert np.array_equal(rec["sum"], np.argwhere(A)) and np.array_equal(rec["lo"], rec["sum"]) and np.array_equal(rec["hi"], rec["sum"])
    check(ctx, A, 0.5, sides=("high",), connectivities=(2, 3), expect_k={2: 1, 3: 1})
    B = ((i // 2 + j // 3 + k // 5) % 2).astype(np.uint8)
    check(ctx, B, 0.5, sides=("high",))


def shells():
    "a box, a cavity in it, a box in the cavity"
    B = np.zeros((12, 12, 70), dtype=np.uint8)
    B[1:11, 1:11, 1:69] = 1
    B[3:9, 3:9, 3:67] = 0
    B[5:7, 5:7, 5:65] = 1
    return B


def test_nested_shells_and_fill_holes(ctx):
    from contourist_amd import volume
    B = shells()
    check(ctx, B, 0.5, expect_k=None)
    for c in (1, 3):
        assert R.label(B, 0.5, "high", c)[1] == 2 and R.label(B, 0.5, "low", c)[1] == 2
        got = volume.fill_holes(B, 0.5, c)
        same(got, R.fill_holes(B, 0.5, c))
        assert got[4, 4, 4] == 1 and got[0, 0, 0] == 0 and got.sum() == 10 * 10 * 68
    # the cavity reaches the rim through corner contacts only: enclosed at connectivity 1, open at 3
    B[2, 2, 2], B[1, 1, 1] = 0, 0
    for c, filled in ((1, 1), (2, 1), (3, 0)):
        got = volume.fill_holes(B, 0.5, c)
        same(got, R.fill_holes(B, 0.5, c))
        assert got[4, 4, 4] == filled and got[2, 2, 2] == filled and got[6, 6, 6] == 1


def test_everything_and_nothing_labelled(ctx):
    from contourist_amd import _ffi
    A = uniform((5, 6, 70), 42)
    check(ctx, A, -1.0, expect_k={1: 1, 2: 1, 3: 1}, sides=("high",))      # nothing is low
    check(ctx, A, -1.0, expect_k={1: 0, 2: 0, 3: 0}, sides=("low",))
    k, got = ctx.label_grid(2.0, "high", 1, samples=A, download=True)
    assert k == 0 and not got.any() and len(ctx.label_measures()) == 0
    assert ctx.lib.cx_grid_label3d_measures(ctx.handle, None, 0) == _ffi.CX_OK      # K == 0 is served with any capacity
    n, mask = ctx.label_select([1], download=True)
    assert n == A.size and mask.all()
    n, mask = ctx.label_select([0], download=True)
    assert n == 0 and not mask.any()
    for keep in ([], [1, 1]):
        with pytest.raises(_ffi.CxError) as e:
            ctx.label_select(keep)
        assert e.value.code == _ffi.CX_ERR_INVALID


@pytest.mark.parametrize("name", ["float32", "uint8", "int8", "uint16", "int16", "float16", "bfloat16"])
def test_sample_types_from_host_and_device(ctx, name):
    import torch
    shape = (4, 9, 67)
    rng = np.random.RandomState(9)
    if name == "bfloat16":
        t = torch.from_numpy((rng.standard_normal(shape) * 3.0).astype(np.float32)).cuda().to(torch.bfloat16)
        values = t.float().cpu().numpy()
        host = (t.view(torch.int16).cpu().numpy().view(np.uint16), "bfloat16", shape)
        value = 1.3
    elif np.dtype(name).kind == "f":
        values = (rng.standard_normal(shape) * 3.0).astype(name)
        t, host, value = torch.from_numpy(values).cuda(), values, 1.3
    else:
        info = np.iinfo(name)
        values = rng.randint(info.min, info.max + 1, size=shape).astype(name)
        values[0, 0, :2] = [info.min, info.max]
        t, host = torch.from_numpy(values).cuda(), values
        value = info.min + 0.7 * (float(info.max) - float(info.min)) + 0.5
    torch.cuda.synchronize()
    check(ctx, values, value, samples=host, connectivities=(1, 3))
    check(ctx, values, value, samples=(t.data_ptr(), t.dtype, shape), connectivities=(2,))
    check(ctx, values, float(values[2, 3, 3]), samples=host, connectivities=(1,))      # a value that is a sample value: f < value is strict


def test_the_low_rule_on_the_device(ctx):
    "NaN (in the high set), infinities, -0.0 against 0.0 and a value between two float32 neighbours"
    A = uniform((4, 5, 70), 13) - 0.5
    A[1, 2, 3], A[2, 3, 60], A[3, 1, 33], A[0, 0, 0], A[0, 0, 1] = np.nan, np.inf, -np.inf, -0.0, 0.0
    A[1] = np.where(A[1] < 0, np.float32(-0.0), np.float32(0.0))
    A[1, 2, 3] = np.nan
    assert R.labelled(A, 0.1, "high")[1, 2, 3] and not R.labelled(A, 0.1, "low")[1, 2, 3]
    for value in (0.0, -0.0, 5e-324, 0.1):
        check(ctx, A, value, connectivities=(1, 3))
    a = np.float32(1.0)
    b = np.nextafter(a, np.float32(2.0))
    B = np.where(uniform((3, 4, 66), 14) < 0.5, a, b).astype(np.float32)
    for value in ((np.float64(a) + np.float64(b)) / 2, np.float64(b), np.nextafter(np.float64(a), 2.0)):
        assert 0 < R.labelled(B, value, "low").sum() < B.size
        check(ctx, B, value, connectivities=(2,))


def test_misaligned_slices_and_callers_output(ctx):
    import torch
    from contourist_amd import _ffi
    shape = (5, 9, 71)
    n = int(np.prod(shape))
    for np_dtype, off in ((np.float32, 1), (np.uint8, 1), (np.int16, 3), (np.uint8, 7)):
        rng = np.random.RandomState(off + 20)
        flat = (rng.uniform(size=n + off) * 100).astype(np_dtype)
        t = torch.from_numpy(flat).cuda()[off:]
        assert t.data_ptr() % 16 != 0
        A = flat[off:].reshape(shape)
        want, k = R.label(A, 60.5, "high", 2)
        for lead in (1, 3):      # elements in front: the output is aligned to its own type and to nothing more
            out = torch.full((n + lead + 2,), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.label_grid(0.5, "high", 1, samples=np.ones((2, 2, 2), dtype=np.uint8))      # pending labels of other samples
            got_k, ptr = ctx.label_grid(60.5, "high", 2, samples=(t.data_ptr(), t.dtype, shape), out=out[lead:].data_ptr())
            host = out.cpu().numpy()
            assert got_k == k and ptr == out[lead:].data_ptr()
            assert np.all(host[:lead] == -7) and np.all(host[lead + n:] == -7)      # nothing written around the labels
            same(host[lead:lead + n].reshape(shape), want)
            with pytest.raises(_ffi.CxError) as e:      # with an output of the caller's the context holds no labels
                ctx.label_result()
            assert e.value.code == _ffi.CX_ERR_STATE
        # masks into every alignment of a caller's buffer
        ctx.label_grid(60.5, "high", 2, samples=(t.data_ptr(), t.dtype, shape))
        keep = keep_pattern(k)
        want_mask, want_n = R.select(want, keep)
        for lead in range(0, 18, off if off > 1 else 1):
            out = torch.full((n + lead + 19,), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            got_n, ptr = ctx.label_select(keep, out=out[lead:].data_ptr())
            host = out.cpu().numpy()
            assert got_n == want_n and ptr == out[lead:].data_ptr()
            assert np.all(host[:lead] == 7) and np.all(host[lead + n:] == 7)
            same(host[lead:lead + n].reshape(shape), want_mask)
            with pytest.raises(_ffi.CxError) as e:
                ctx.label_mask_result()
            assert e.value.code == _ffi.CX_ERR_STATE
    # a mask shorter than one 16-byte group
    small = np.asarray([[[1, 0, 1, 1, 0]]], dtype=np.uint8)
    ctx.label_grid(0.5, samples=small)
    out = torch.full((9,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.label_select([0, 1, 0], out=out[2:].data_ptr())[0] == 1
    assert out.cpu().numpy().tolist() == [7, 7, 1, 0, 0, 0, 0, 7, 7]


def test_two_calls_give_the_same_bytes(ctx):
    A = uniform(STRADDLE, 17)
    results = []
    for _ in range(2):
        k, labels = ctx.label_grid(0.69, "high", 1, samples=A, download=True)
        rec = ctx.label_measures()
        n, mask = ctx.label_select(keep_pattern(k), download=True)
        results.append((k, labels.tobytes(), rec.tobytes(), n, mask.tobytes()))
        k2, _ = ctx.label_grid(0.5, "low", 3, samples=uniform((3, 3, 70), 1), download=True)      # (the scratch is reused in between)
        ctx.label_measures()
        ctx.label_select(np.ones(k2 + 1), download=True)
    assert results[0] == results[1]


def quantised_noise():
    A = np.load(os.path.join(GOLDEN_DIR, "noise32_v0.npz"))["A"]
    lo, hi = float(A.min()), float(A.max())
    return np.clip(np.rint((A - lo) * (255.0 / (hi - lo))), 0, 255).astype(np.uint8)


def march_both_routes(U, device_route, host_grid, value):
    "the Level-0 mesh of the grid `device_route(context)` leaves bound == that of `host_grid` uploaded"
    from contourist_amd import _ffi
    meshes = []
    for route in ("device", "host"):
        c = _ffi.Context()
        try:
            if route == "device":
                c.upload_grid_native(U)
                assert c.grid_info() == dict(dtype="uint8", device_bytes=U.size)
                device_route(c)
                assert c.shape == U.shape
            else:
                c.upload_grid_native(host_grid)
            assert c.grid_info() == dict(dtype=host_grid.dtype.name, device_bytes=host_grid.nbytes)
            counts = c.extract3d(value, _ffi.CX_DIAG_CPYTHON310)
            meshes.append((counts, c.download_level0_records(counts)))
        finally:
            c.close()
    (c0, m0), (c1, m1) = meshes
    assert c0 == c1 and c0["n_triangles"] > 1000
    assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1].view(np.uint32), m1[1].view(np.uint32)) and np.array_equal(m0[2], m1[2])


def test_upload_label_keep_the_largest_bind_march():
    "a uint8 volume is uploaded, its largest object kept and marched with no array of the volume's size on the host"
    U = quantised_noise()
    want = R.keep_components(U, 127.3, largest=1)

    def route(c):
        k, ptr = c.label_grid(127.3, "high")      # the bound grid in, the context's own buffer out
        assert c.label_result() == (U.shape, ptr, "high", 1, k)
        rec = c.label_measures()
        keep = np.zeros(k + 1, dtype=np.uint8)
        keep[1 + int(np.argmax(rec["voxels"]))] = 1
        n, mptr = c.label_select(keep)
        assert n == int(want.sum()) and c.label_mask_result() == (U.shape, mptr, n)
        c.bind_label_mask()

    march_both_routes(U, route, want, 0.5)


def test_upload_fill_holes_signed_distance_bind_march():
    "the mask of a select is the input of the distance transform where it lies"
    U = quantised_noise()
    filled = R.fill_holes(U, 127.3, 1)
    assert filled.sum() > (U >= 127.3).sum()      # there are holes to fill

    def route(c):
        k, _ = c.label_grid(127.3, "low", 1)
        rec = c.label_measures()
        n, mptr = c.label_select(np.concatenate([[1], rec["rim"] == 0]))
        assert n == int(filled.sum())
        sites, _ = c.distance_grid(0.5, "signed", samples=(mptr, "uint8", U.shape))
        assert sites == D.n_sites(filled, 0.5, "signed")
        c.bind_distance()
        assert c.label_mask_result() == (U.shape, mptr, n)      # the mask was read, not taken

    march_both_routes(U, route, D.distance(filled, 0.5, "signed"), 0.0)


def test_volume_module(ctx):
    import torch
    from contourist_amd import volume
    A = uniform((12, 21, 70), 15)
    U = (uniform((12, 21, 70), 16) * 255).astype(np.uint8)
    for S, value in ((A, 0.69), (U, 200.5)):
        t = torch.from_numpy(S).cuda()
        for c in (1, 2, 3):
            want, k = R.label(S, value, "high", c)
            rec = R.records(want, k)
            for src in (S, t):
                out = volume.label(src, value, connectivity=c)
                assert out[1] == k and len(out) == 2
                labels, kk, got_rec = volume.label(src, value, "high", c, measures=True)
                assert kk == k
                same_records(got_rec, rec)
                if src is t:
                    assert labels.is_cuda and labels.dtype == torch.int32 and out[0].is_cuda
                    labels, out = labels.cpu().numpy(), (out[0].cpu().numpy(), k)
                same(labels, want)
                same(out[0], want)
        low, k_low = volume.label(S, value, "low", 2)
        same(low, R.label(S, value, "low", 2)[0])
        sizes = R.records(*R.label(S, value, "high", 1))["voxels"]
        choices = [dict(largest=1), dict(largest=3), dict(min_voxels=4), dict(rim=True), dict(rim=False), dict(min_voxels=3, rim=False, largest=2),
                   dict(keep=(sizes % 2 == 0)), dict(keep=lambda r: r["lo"][:, 2] > 10), dict(keep=lambda r: r["voxels"] < 5, rim=True, largest=4),
                   dict(side="low", connectivity=3, rim=False), dict(largest=0)]
        for kw in choices:
            want = R.keep_components(S, value, **kw)
            same(volume.keep_components(S, value, **kw), want)
            got = volume.keep_components(t, value, **kw)
            assert got.is_cuda and got.dtype == torch.uint8
            same(got.cpu().numpy(), want)
        for c in (1, 3):
            for src in (S, t):
                for fn, ref, args in ((volume.remove_small, R.remove_small, (5,)), (volume.clear_border, R.clear_border, ()), (volume.fill_holes, R.fill_holes, ())):
                    got = fn(src, value, *args, connectivity=c)
                    same(got.cpu().numpy() if src is t else got, ref(S, value, *args, connectivity=c))
    # `largest` with a tie: two components of 4 voxels and one of 3; the smaller label wins
    T = np.zeros((3, 5, 70), dtype=np.uint8)
    T[0, 0, 60:64], T[1, 2, 62:66], T[2, 4, 0:3] = 1, 1, 1
    got = volume.keep_components(T, 0.5, largest=1)
    same(got, R.keep_components(T, 0.5, largest=1))
    assert got[0, 0, 60] == 1 and got[1, 2, 62] == 0 and got.sum() == 4
    assert volume.keep_components(T, 0.5, largest=2).sum() == 8
    # bool masks, two dimensions and one; the rim of a 2-D array is its own
    M = uniform((30, 70), 18) < 0.55
    for c in (1, 2):
        want, k = R.label(M, 0.5, "high", c)
        labels, kk, rec = volume.label(M, 0.5, connectivity=c, measures=True)
        assert kk == k and labels.shape == M.shape
        same(labels, want)
        same_records(rec, R.records(want, k))
        same(volume.fill_holes(M, 0.5, c), R.fill_holes(M, 0.5, c))
        same(volume.clear_border(M, 0.5, c), R.clear_border(M, 0.5, c))
        same(volume.clear_border(torch.from_numpy(M).cuda(), 0.5, c).cpu().numpy(), R.clear_border(M, 0.5, c))
    assert 0 < volume.clear_border(M, 0.5, 1).sum() < M.sum()
    row = M[7]
    labels, k = volume.label(row, 0.5)
    same(labels, R.label(row, 0.5)[0])
    assert k == R.label(row, 0.5)[1] and labels.shape == row.shape
    same(volume.remove_small(row, 0.5, 2), R.remove_small(row, 0.5, 2))
    # float64 samples are rounded to float32 first
    same(volume.label(A.astype(np.float64) + 1e-12, 0.69)[0], R.label((A.astype(np.float64) + 1e-12).astype(np.float32), 0.69)[0])


def test_a_call_leaves_the_state_and_binding_resets_it():
    from contourist_amd import _ffi
    A = np.random.RandomState(19).standard_normal((12, 13, 70)).astype(np.float32)
    axes = [(np.asarray([0.25, 0.5, 0.25], dtype=np.float32), 1, 1)] * 3
    before_bytes = _ffi.device_bytes()[0]
    c = _ffi.Context()
    try:
        c.upload_grid(A)
        counts = c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310)
        l0 = c.download_level0_records(counts)
        cap = c.cap3d()
        cap_mesh = c.download_cap(cap)
        p = c.postprocess3d()
        l1 = c.download_level1(p)
        filt = c.filter_grid(axes)                                                # a pending filter result
        n_sites, dptr = c.distance_grid(0.1, "signed")                            # a pending distance field
        dist = c.distance_result()
        k, lptr = c.label_grid(0.1, "high", 2)                                    # of the bound grid, into the context
        c.label_measures()
        n, mptr = c.label_select(keep_pattern(k))
        c.label_grid(0.5, samples=np.zeros((5, 6, 7), dtype=np.uint8), out=None, download=True)      # of other samples
        assert c.counts() == counts and c.grid_info() == dict(dtype="float32", device_bytes=A.size * 4)
        assert all(np.array_equal(a, b) for a, b in zip(l0, c.download_level0_records(counts)))
        assert all(np.array_equal(a, b) for a, b in zip(l1, c.download_level1(p)))
        assert all(np.array_equal(a, b) for a, b in zip(cap_mesh, c.download_cap(cap)))
        assert c.filter_result() == filt and c.distance_result() == dist
        assert c.extract3d(0.1, _ffi.CX_DIAG_CPYTHON310) == counts               # the grid is the one uploaded
        levels = c.extract3d_levels([-0.4, 0.1, 0.6], _ffi.CX_DIAG_CPYTHON310)
        c.select_level(1)
        sel = c.download_level0_records(levels[1])
        k, lptr = c.label_grid(0.1, "high", 2)
        want, want_k = R.label(A, 0.1, "high", 2)
        assert k == want_k
        n, mptr = c.label_select(keep_pattern(k))
        assert c.counts() == levels[1]
        assert all(np.array_equal(a, b) for a, b in zip(sel, c.download_level0_records(levels[1])))
        c.select_level(2)
        assert c.counts() == levels[2]
        cap = c.cap3d()
        p = c.postprocess3d()
        # the filter and the distance transform do not disturb the pending labels and mask either
        filt = c.filter_grid(axes)
        c.distance_grid(0.1, "signed")
        dist = c.distance_result()
        assert c.label_result() == (A.shape, lptr, "high", 2, k) and c.label_mask_result() == (A.shape, mptr, n)
        same_records(c.label_measures(), R.records(want, k))
        # bind: as after an upload; the filter's and the distance transform's results and the labels stay
        c.bind_label_mask()
        for gone in (c.counts, lambda: c.select_level(0), lambda: c.download_level1(p), c.label_mask_result, c.bind_label_mask, lambda: c.download_cap(cap)):
            with pytest.raises(_ffi.CxError) as e:
                gone()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert c.filter_result() == filt and c.distance_result() == dist
        assert c.label_result() == (A.shape, lptr, "high", 2, k)
        same_records(c.label_measures(), R.records(want, k))
        assert c.shape == A.shape and c.grid_info() == dict(dtype="uint8", device_bytes=A.size)
        again = c.extract3d(0.5, _ffi.CX_DIAG_CPYTHON310)
        fresh = _ffi.Context()
        try:
            fresh.upload_grid_native(R.select(want, keep_pattern(k))[0])
            assert fresh.extract3d(0.5, _ffi.CX_DIAG_CPYTHON310) == again
        finally:
            fresh.close()
        # a second mask of the labels that stayed, bound again: the grid owned before is released
        live = _ffi.device_bytes(c.handle)[0]
        c.label_select(1 - keep_pattern(k))
        c.bind_label_mask()
        assert _ffi.device_bytes(c.handle)[0] == live
        # the bound mask labelled itself (no samples given), and the pending mask as the samples of a label call
        k2, _ = c.label_grid(0.5, "high", 1)
        assert k2 == R.label(R.select(want, 1 - keep_pattern(k))[0], 0.5, "high", 1)[1]
        n, mptr = c.label_select(np.ones(k2 + 1))
        assert n == A.size
        k3, got = c.label_grid(0.5, "high", 3, samples=(mptr, "uint8", A.shape), download=True)
        assert k3 == 1 and np.all(got == 1)
        # a mask the march does not take stays pending
        thin = np.zeros((1, 13, 70), dtype=np.uint8)
        thin[0, 4, 5] = 1
        c.label_grid(0.5, samples=thin)
        n, mptr = c.label_select([0, 1])
        with pytest.raises(_ffi.CxError) as e:
            c.bind_label_mask()
        assert e.value.code == _ffi.CX_ERR_INVALID and c.label_mask_result() == ((1, 13, 70), mptr, 1) and c.shape == A.shape
    finally:
        c.close()
    assert _ffi.device_bytes()[0] == before_bytes


def test_errors(ctx):
    import torch
    from contourist_amd import _ffi
    A = uniform((4, 5, 6), 21)

    def code(value=0.5, side="high", connectivity=1, samples=A, **kw):
        with pytest.raises(_ffi.CxError) as e:
            ctx.label_grid(value, side, connectivity, samples=samples, **kw)
        return e.value.code

    fresh = _ffi.Context()
    try:
        calls = (lambda: fresh.label_grid(0.5), fresh.label_result, fresh.label_measures, lambda: fresh.label_select([1]), fresh.label_mask_result,
                 fresh.bind_label_mask)
        for call in calls:
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
        fresh.label_grid(0.5, samples=A)      # labels, but no mask yet
        for call in (fresh.label_mask_result, fresh.bind_label_mask):
            with pytest.raises(_ffi.CxError) as e:
                call()
            assert e.value.code == _ffi.CX_ERR_STATE
        assert fresh.lib.cx_grid_label3d_measures(fresh.handle, None, 0) == _ffi.CX_ERR_INVALID      # K > 0
    finally:
        fresh.close()
    for value in (float("nan"), float("inf"), -float("inf")):
        assert code(value=value) == _ffi.CX_ERR_INVALID
    for connectivity in (0, 4, -1):
        assert code(connectivity=connectivity) == _ffi.CX_ERR_INVALID
    _ffi.LABEL_SIDES["inside"] = 2
    try:
        assert code(side="inside") == _ffi.CX_ERR_INVALID
    finally:
        del _ffi.LABEL_SIDES["inside"]
    t = torch.from_numpy(A).cuda()
    torch.cuda.synchronize()
    dev = (t.data_ptr(), t.dtype, A.shape)
    call = ctx.lib.cx_grid_label3d
    for dtype in (7, -1):
        assert call(ctx.handle, t.data_ptr(), dtype, 1, 4, 5, 6, 0.5, 0, 1, None, None, None) == _ffi.CX_ERR_INVALID
    for shape in ((0, 5, 6), (4, -1, 6), (1 << 15, 1 << 15, 1)):      # an empty axis, and more than 2^29 samples
        assert call(ctx.handle, t.data_ptr(), 0, 1, shape[0], shape[1], shape[2], 0.5, 0, 1, None, None, None) == _ffi.CX_ERR_INVALID
    assert call(None, t.data_ptr(), 0, 1, 4, 5, 6, 0.5, 0, 1, None, None, None) == _ffi.CX_ERR_INVALID
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
    want, k = R.label(A, 0.5, "high", 1)
    assert ctx.label_grid(0.5, samples=src, out=big.data_ptr())[0] == k
    same(big[:A.size].view(torch.int32).cpu().numpy().reshape(A.shape), want)
    # the records: room for fewer than K; the select: another n_keep, an output that overlaps the labels
    k, lptr = ctx.label_grid(0.5, samples=dev)
    assert k == R.label(A, 0.5)[1] and k >= 2
    room = np.zeros(k, dtype=_ffi.LABEL_COMPONENT_DTYPE)
    assert ctx.lib.cx_grid_label3d_measures(ctx.handle, room.ctypes.data, k - 1) == _ffi.CX_ERR_INVALID
    assert ctx.lib.cx_grid_label3d_measures(ctx.handle, room.ctypes.data, k) == _ffi.CX_OK
    same_records(room, R.records(want, k))
    for keep in (np.ones(k), np.ones(k + 2), []):
        with pytest.raises(_ffi.CxError) as e:
            ctx.label_select(keep)
        assert e.value.code == _ffi.CX_ERR_INVALID
    for out in (lptr, lptr + 4 * A.size - 1, lptr - A.size + 1):
        with pytest.raises(_ffi.CxError) as e:
            ctx.label_select(np.ones(k + 1), out=out)
        assert e.value.code == _ffi.CX_ERR_INVALID
    assert ctx.label_result() == (A.shape, lptr, "high", 1, k)      # the refused calls changed nothing


def test_a_pointer_into_the_pending_result():
    "planes 1 to 5 of the pending mask of a selection as the samples of the next call, whose selection writes the context's mask again"
    from contourist_amd import _ffi
    A = uniform((6, 9, 70), 41)
    labels, k = R.label(A, 0.6, "high", 1)
    keep = keep_pattern(k)
    keep[0] = 0      # two components of three, and none of the unlabelled samples
    first = R.select(labels, keep)[0]
    assert k >= 2 and 0 < first[1:].sum() < first[1:].size
    c = _ffi.Context()
    try:
        c.label_grid(0.6, "high", 1, samples=A)
        _, mptr = c.label_select(keep)
        k2, got = c.label_grid(0.5, "high", 2, samples=(mptr + 9 * 70, "uint8", (5, 9, 70)), download=True)
        want, want_k = R.label(first[1:], 0.5, "high", 2)
        assert k2 == want_k >= 2
        same(got, want)
        n, mask = c.label_select(keep_pattern(k2), download=True)
        want_mask, want_n = R.select(want, keep_pattern(k2))
        assert n == want_n
        same(mask, want_mask)
        assert c.label_result()[::2] == ((5, 9, 70), "high", k2) and c.label_mask_result()[::2] == ((5, 9, 70), n)
    finally:
        c.close()
