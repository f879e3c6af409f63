"""GPU: the back half of config 4 at full size against an independent oracle chain.

BASELINE config 4 is the 128^3 x 64 moving-blobs field (contourist_amd.synthetic.moving_blobs_torch, seed 1236, isovalue CONFIG4_VALUE).
tests/test_gpu_bench_fields.py holds its Level-0 march to the C oracle; this module holds what bench.py runs after it:
cx_postprocess4d (B3), cx_morph_triangles (B4, B5) and cx_morph_eval_many (B6, 64 surfaces).  The chain on the host is the C oracle's
Level 0 (oracle/level0_4d.march4d), oracle/postpass4d.find_tetrahedra_post, collect_morph_triangles_np and morph_eval.SurfaceStream;
the numpy oracles are held to the loop restatements of the reference by tests/test_oracle4d_np.py.

Only this size reaches the paths a small field cannot: edge tables sized from the pair count, single-workgroup scans over tens of
thousands of block sums, segment ids by ordered compaction over many blocks, the start-time sort over 256 bins, per-time windows
that span many blocks, and the descriptors of more than 1 151 times outside pinned memory."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def check_post_and_morph(keys, host, value, points_post, tets_post, post, morph):
    """B3 and B4 of the device against the oracle chain run on `host` (the same samples): counts, float64 points in key order bit
    for bit, the canonical tetrahedron set, directed segments and triangles as sets of edge keys.  -> the oracle's morph dict"""
    from oracle import level0_4d, postpass4d
    kh = np.asarray(keys, dtype=np.int64)
    O = level0_4d.march4d(host, value, diag_mode=1, vcap=len(kh) + 4096, tcap=8 * len(kh) + 4096)   # (grows by itself if need be)
    ko = level0_4d.edge_keys4(O["pairs"], host.shape)
    del O["pairs"]
    assert len(ko) == len(kh)
    W = postpass4d.find_tetrahedra_post(ko, O["xyzt"], O["tets"], np.array(host.shape) - 1)
    del O
    # ---- B3: bin_times / drop_instant / tiny collapse
    assert post["n_after_drop"] == W["n_after_drop"] and post["n_after_tiny"] == W["n_after_tiny"]
    assert len(tets_post) == W["n_after_tiny"]
    od, oo = np.argsort(kh), np.argsort(ko)
    assert np.array_equal(kh[od], ko[oo])
    assert np.array_equal(points_post[od].view(np.uint64), W["xyzt"][oo].view(np.uint64)), "post-step points differ from the oracle"
    got = level0_4d.canonical4(kh, points_post, tets_post.astype(np.int64))[2]
    want = level0_4d.canonical4(ko, W["xyzt"], W["tets"])[2]
    assert np.array_equal(got, want), "post-step tetrahedra differ from the oracle"
    del got, want
    # ---- B4: the slicing into morph triangles
    M = postpass4d.collect_morph_triangles_np(ko, W["xyzt"], W["tets"])
    del W
    pts, segs, tris = morph[:3]
    assert np.array_equal(pts.view(np.uint64), points_post.view(np.uint64))       # the morph triangles' points are the post steps'
    assert len(segs) == len(M["segments"]) and len(tris) == len(M["triangles"]), (len(segs), len(M["segments"]), len(tris), len(M["triangles"]))
    mk = M["keys"]

    def rows(a):
        return a[np.lexsort(a.T[::-1])]
    sd = rows(kh[np.asarray(segs, dtype=np.int64)])                   # directed: low t -> high t
    so = rows(mk[M["segments"]])
    assert np.array_equal(sd, so), "morph segments differ from the oracle"
    # triangles as sets of segments, a segment as its sorted pair of edge keys: segment -> its rank among the oracle's sorted pairs
    code_o = np.sort(mk[M["segments"]], axis=1)
    rank_o = np.lexsort(code_o.T[::-1])
    pos_o = np.empty(len(rank_o), dtype=np.int64)
    pos_o[rank_o] = np.arange(len(rank_o))
    code_d = np.sort(kh[np.asarray(segs, dtype=np.int64)], axis=1)
    rank_d = np.lexsort(code_d.T[::-1])
    assert np.array_equal(code_d[rank_d], code_o[rank_o])
    pos_d = np.empty(len(rank_d), dtype=np.int64)
    pos_d[rank_d] = np.arange(len(rank_d))
    td = rows(np.sort(pos_d[np.asarray(tris, dtype=np.int64)], axis=1))
    to = rows(np.sort(pos_o[M["triangles"]], axis=1))
    assert np.array_equal(td, to), "morph triangles differ from the oracle"
    return M


def in_id_order(W):
    """a viewer surface (oracle order: active triangles by (tr_min, id), points numbered by first use) in the order the device writes
    it: triangles by id, points by segment id -> (points, faces)"""
    seg = np.asarray(W["segment_ids"], dtype=np.int64)
    by_id = np.argsort(seg)
    renum = np.empty(len(seg), dtype=np.int64)
    renum[by_id] = np.arange(len(seg))
    keep = np.argsort(np.asarray(W["active"], dtype=np.int64), kind="stable")
    return W["points"][by_id], renum[W["faces"][keep]]


def check_surfaces(stream, times, surfaces):
    "B6: every device surface equals the viewer oracle's, faces exactly, points within 1e-12 -> total triangles"
    total = 0
    for i, t in enumerate(times):
        pw, fw = in_id_order(stream.surface_at(float(t)))
        pm, tm = surfaces[i]
        assert len(tm) == len(fw) and len(pm) == len(pw), (i, t, len(tm), len(fw), len(pm), len(pw))
        assert np.array_equal(tm, fw), (i, t)
        assert np.allclose(pm, pw, rtol=0, atol=1e-12), (i, t, float(np.abs(pm - pw).max()))
        total += len(tm)
    return total


def test_config4_back_half_against_the_oracle():
    """B3 post steps, B4 morph triangles, B5 windings of all 64 surfaces, B6 the per-t stream (bench.py's 64 times, vertex times,
    times outside the range, single calls, and more than 1 151 times in one call) on the 128^3 x 64 bench field"""
    torch = pytest.importorskip("torch")
    from contourist_amd import _ffi, synthetic
    from oracle import morph_eval
    from test_gpu_fullsize import edge_consistency
    dev = torch.device("cuda", 0)
    shape = (128, 128, 128, 64)
    value = synthetic.CONFIG4_VALUE
    A = synthetic.moving_blobs_torch(shape, 1236, dev)
    host = np.ascontiguousarray(A.cpu().numpy())
    ctx = _ffi.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    try:
        ctx.adopt_device_grid4d(A.data_ptr(), shape, keepalive=A)
        c = ctx.extract4d(value, _ffi.CX_DIAG_CPYTHON310)
        _, keys, _ = ctx.download_level0_4d(c)
        post = ctx.postprocess4d(100)
        points_post, tets_post = ctx.download_level1_4d(post)
        morph = ctx.morph_triangles()
        pts, segs, tris, _ = morph
        assert len(tris) > 2e7 and len(segs) > 1e7
        tmin, tmax = float(pts[:, 3].min()), float(pts[:, 3].max())
        bench_times = np.linspace(tmin, tmax, shape[3])                          # bench.py run_config4
        vt = np.unique(pts[:, 3])
        extra = np.array([vt[1], vt[len(vt) // 3], vt[len(vt) // 2], vt[-2], tmin - 1.0, tmax + 0.5])
        times = np.concatenate([bench_times, extra])
        many = ctx.morph_eval_many(times)
        many = [(p.copy(), t.copy()) for p, t in many]
        # single calls: the same arrays as the batched call
        for i in (0, 17, 40, shape[3] - 1, shape[3] + 1):
            p1, t1 = ctx.morph_eval(float(times[i]))
            assert np.array_equal(t1, many[i][1]) and np.array_equal(p1, many[i][0]), i
        # more than 1 151 times: the descriptors and totals outside the pinned staging; the bench times among times outside the range
        rng = np.random.RandomState(4)
        outside = np.concatenate([tmin - 1.0 - 1e-3 * np.arange(600), tmax + 0.5 + 1e-3 * np.arange(600)])
        big = np.concatenate([outside, bench_times])
        perm = rng.permutation(len(big))
        big = big[perm]
        counts = ctx.morph_eval_many(big, download=False)
        assert len(big) > 1151 and counts.shape == (len(big), 2)
        where = np.empty(len(big), dtype=np.int64)
        where[perm] = np.arange(len(big))
        for j in range(len(big)):
            k = perm[j]
            if k < len(outside):
                assert counts[j, 0] == 0 and counts[j, 1] == 0
        for i in range(shape[3]):
            j = where[len(outside) + i]
            pi = np.empty((int(counts[j, 0]), 3), dtype=np.float64)
            ti = np.empty((int(counts[j, 1]), 3), dtype=np.int32)
            ctx._check(ctx.lib.cx_morph_eval_many_download(ctx.handle, int(j), pi.ctypes.data, ti.ctypes.data))
            assert np.array_equal(ti, many[i][1]) and np.array_equal(pi, many[i][0]), i
    finally:
        ctx.close()
        del A
        torch.cuda.empty_cache()
    # ---- B5: every time slice is consistently wound (no manifold edge run twice in the same direction)
    for i in range(shape[3]):
        tm = many[i][1]
        if len(tm):
            manifold, same, other = edge_consistency(tm)
            assert same == 0, (i, manifold, same)
    assert sum(len(many[i][1]) > 100000 for i in range(shape[3])) > 50
    # ---- B3 / B4 against the oracle chain
    check_post_and_morph(keys, host, value, points_post, tets_post, post, morph)
    del host, tets_post
    # ---- B6 against the viewer oracle on the device's morph triangles
    stream = morph_eval.SurfaceStream(pts, segs, tris)
    total = check_surfaces(stream, times, many)
    assert total > 1.5e7
    assert len(many[shape[3] - 1][1]) == 0 and len(many[-1][1]) == 0 and len(many[-2][1]) == 0    # at tmax and outside: nothing lives
