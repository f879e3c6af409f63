"""GPU: the branches of the 4-D Level-0 kernels (csrc/cx_march4d.hip) that only large grids reach, at small sizes, and the inputs
that so far only tools/fuzz_gpu4d.py drew -- every mesh against oracle/level0_4d.march4d exactly as check() of test_gpu_level0_4d.py
compares (crossing-edge keys and tetrahedron key quadruples exact, the three counts exact, coordinates within 1e-6 |x| + 1e-6).

Cases under launch knobs (CX4_IPB, CX4_CELLS_WGS, CX4_TETS_WGS, CX4_SB_BLOCKS, CX4_SB_ROWS: honoured only in a process started with
CX_DEBUG=1) run in one child process per knob setting.  Before the GPU is touched every such case proves ON THE CPU that its input
reaches the branch it is about: active cells as cx_k_queue4 defines them, grouped by bitmap word, walked the way the kernel's
waves walk them (KNOB_CASES[...]["cond"]; tests/test_march4d_paths_inputs.py runs the same conditions without a GPU and requires
each to fail with its knob back at the default)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_level0_4d import check

import setorder4d_cases

pytestmark = pytest.mark.gpu

CX4_QCAP, CX4_WCAP = 2048, 128        # cx_march4d.hip: cells / bitmap words a wave of cx_k_queue4 stages in LDS
MODES = (("cpython310", 1), ("canonical", 0))


# ---- fields ------------------------------------------------------------------------------------------------------------------
def noise(shape, seed):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


def smoothed(A, passes):
    A = np.asarray(A, dtype=np.float64)
    for _ in range(passes):
        for ax in range(4):
            A = 0.25 * np.roll(A, 1, ax) + 0.5 * A + 0.25 * np.roll(A, -1, ax)
    return (A / max(A.std(), 1e-9)).astype(np.float32)


def quarters(A):
    return (np.round(A * 4) / 4).astype(np.float32)


# ---- the comparison where check() cannot make it: an origin, a context used again, an adopted device array, the async entry -------
_ORACLE = {}


def oracle_canon(A, v, diag_mode, origin=(0, 0, 0, 0), key=None):
    "the oracle's mesh in canonical form (computed once per key and left unchanged)"
    from oracle import level0_4d
    k = None if key is None else (key, float(v), np.signbit(v), diag_mode, tuple(origin))
    if k is not None and k in _ORACLE:
        return _ORACLE[k]
    O = level0_4d.march4d(A, v, diag_mode=diag_mode, origin=origin)
    ko = level0_4d.edge_keys4(O["pairs"], A.shape)
    out = (level0_4d.canonical4(ko, O["xyzt"], O["tets"]), len(ko), len(O["tets"]), O["nborder_mixed"])
    if k is not None:
        _ORACLE[k] = out
    return out


def check_ctx(ctx, A, v, diag_mode, origin=(0, 0, 0, 0), key=None, use_async=False, adopt=None):
    """check() with the context in the caller's hands.  adopt: a contiguous float32 device tensor holding A (cx_grid4d_adopt_device)
    instead of the upload."""
    from contourist_amd import _ffi
    from oracle import level0_4d
    co, nv, nt, nb = oracle_canon(A, v, diag_mode, origin, key)
    flags = _ffi.CX_DIAG_CPYTHON310 if diag_mode else _ffi.CX_DIAG_CANONICAL
    ctx.set_origin4d(*origin)
    try:
        if adopt is not None:
            ctx.adopt_device_grid4d(adopt.data_ptr(), A.shape, keepalive=adopt)
        else:
            ctx.upload_grid4d(A)
        if use_async:
            ctx.extract4d_async(v, flags)
            c = ctx.counts4d()
        else:
            c = ctx.extract4d(v, flags)
        verts, keys, tets = ctx.download_level0_4d(c)
    finally:
        ctx.set_origin4d(0, 0, 0, 0)
    assert c["n_vertices"] == nv and c["n_tetrahedra"] == nt
    assert c["n_border_voxels"] == nb
    ch = level0_4d.canonical4(keys.astype(np.int64), verts, tets.astype(np.int64))
    assert np.array_equal(co[0], ch[0])
    assert np.all(np.abs(ch[1] - co[1]) <= 1e-6 * np.abs(co[1]) + 1e-6)
    assert np.array_equal(co[2], ch[2])
    return c, ch


def check_both(A, v):
    n = 0
    for diagonal, mode in MODES:
        R, _ = check(A, v, diagonal, mode)
        n += R["counts"]["n_tetrahedra"]
    return n


# ---- what the kernels do with an input, on the CPU ------------------------------------------------------------------------------
def vcmp32(v):
    "smallest fp32 >= v: (double)f < v  <=>  f < vcmp (for the isovalues of the knob cases simply np.float32(v))"
    t = np.float32(v)
    return np.nextafter(t, np.float32(np.inf)) if float(t) < float(v) else t


def active_cells(A, v):
    "cx_k_queue4's active cells: the 16 corners, clamped onto the array, are not all on one side of A < np.float32(v)"
    low = np.asarray(A, dtype=np.float32) < vcmp32(v)
    P = np.pad(low, [(0, 1)] * 4, mode="edge")
    n = A.shape
    any_, all_ = np.zeros(n, bool), np.ones(n, bool)
    for c in range(16):
        s = P[(c >> 3) & 1:, (c >> 2) & 1:, (c >> 1) & 1:, c & 1:][:n[0], :n[1], :n[2], :n[3]]
        any_ |= s
        all_ &= s
    return any_ & ~all_


def word_counts(act):
    "active cells per item of cx_k_queue4: one bitmap word = 32 cells of one row"
    n3 = act.shape[3]
    nw3 = (n3 + 31) // 32
    rows = act.reshape(-1, n3)
    pad = np.zeros((rows.shape[0], nw3 * 32), bool)
    pad[:, :n3] = rows
    return pad.reshape(-1, 32).sum(axis=1)


def knob(env, name, default):
    "cx_debug_knob: the value only with CX_DEBUG=1 and when positive"
    if env.get("CX_DEBUG") != "1":
        return default
    try:
        x = int(env.get(name, "0"))
    except ValueError:
        x = 0
    return x if x > 0 else default


def queue_ipb(env, nitems):
    "cx_launch_classify4d: items per workgroup of cx_k_queue4"
    ipb = knob(env, "CX4_IPB", (nitems + 3071) // 3072)
    return max(256, (ipb + 255) & ~255)


def queue_flushes(words, ipb):
    """the flushes of cx_k_queue4's waves before their final one: wave w of workgroup blk takes items [blk ipb + 64 w + 256 s, + 64)
    in step s and flushes first when the step does not fit.  -> {(blk, wave): ["Q" | "W" | "QW", ...]}, the side(s) that overflowed"""
    nitems = len(words)
    out = {}
    for blk in range((nitems + ipb - 1) // ipb):
        gend = min((blk + 1) * ipb, nitems)
        for w in range(4):
            qn = wn = 0
            why = []
            g = blk * ipb + 64 * w
            while g < gend:
                part = words[g:min(g + 64, gend)]
                tot, nwords = int(part.sum()), int((part > 0).sum())
                if qn + tot > CX4_QCAP or wn + nwords > CX4_WCAP:
                    why.append(("Q" if qn + tot > CX4_QCAP else "") + ("W" if wn + nwords > CX4_WCAP else ""))
                    qn = wn = 0
                qn += tot
                wn += nwords
                g += 256
            if why:
                out[(blk, w)] = why
    return out


def flushes_of(A, v, env):
    words = word_counts(active_cells(A, v))
    return queue_flushes(words, queue_ipb(env, len(words)))


def fresh_qcap(A):
    "queue entries a fresh context reserves (cx_api4d.hip begin4): the launchers size the later stages' grids by it"
    return A.size // 8 + 4096


def cells_wgs(env, A):
    return min((fresh_qcap(A) + 511) // 512, knob(env, "CX4_CELLS_WGS", 1024))


def tets_rounds(env, A, v):
    "cx_k_emit_tets: (rounds, whole rounds, rounds that run as two halves) for the waves of its grid"
    nwaves = 4 * min((fresh_qcap(A) + 255) // 256, knob(env, "CX4_TETS_WGS", 1024))
    nrounds = (int(active_cells(A, v).sum()) + 63) // 64
    nfull = (nrounds // nwaves) * nwaves
    return nrounds, nfull, nrounds - nfull


def signbits_trips(env, A):
    "trips of the busiest wave's grid-stride loop in the sign-bitmap kernel that runs for A (cx_launch_signbits4d); -> (kernel, trips)"
    n3 = A.shape[3]
    cap = knob(env, "CX4_SB_BLOCKS", 0)
    if n3 % 32 == 0 and not knob(env, "CX4_SB_ROWS", 0):
        nquads = A.size // 4
        blocks = min((nquads + 2047) // 2048, 256 * knob(env, "CX4_SB_WGS", 16))
        blocks = min(blocks, cap) if cap else blocks
        return "flat", (nquads + blocks * 2048 - 1) // (blocks * 2048)
    total = (A.size // n3) * ((n3 + 63) // 64)
    blocks = min(((total + 7) // 8 + 3) // 4, 256 * 64)
    blocks = min(blocks, cap) if cap else blocks
    return "rows", (total + blocks * 32 - 1) // (blocks * 32)


# ---- the cases under knobs ---------------------------------------------------------------------------------------------------
def f_qcap():
    return noise((4, 4, 16, 64), 101), 0.1


def f_wcap():
    return noise((8, 8, 12, 3), 102), 0.1


def f_both():
    return quarters(smoothed(noise((6, 8, 16, 65), 103), 2)), 0.25


def f_cells():
    return noise((9, 8, 7, 10), 104), 0.1


# white noise trimmed until the queued cells give these round counts with 4 waves (CX4_TETS_WGS=1): rounds % 4 = 0, 1, 3 with whole
# rounds before them, 2 as well, a row that crosses bitmap words (41 rounds), and one with fewer rounds than waves (all halves)
TETS_SHAPES = (((4, 4, 5, 6), 8), ((4, 4, 4, 9), 9), ((4, 5, 5, 7), 11), ((5, 5, 5, 5), 10), ((4, 4, 5, 33), 41), ((3, 3, 4, 5), 3))


def f_tets(shape):
    return noise(shape, 200 + sum(shape)), 0.1


SB_ROW_SHAPES = ((5, 4, 3, 70), (3, 3, 4, 600), (5, 3, 3, 70))      # the third: 90 chunks, the last group of 8 is clamped
SB_FLAT_SHAPES = ((6, 5, 4, 64), (7, 5, 5, 64))                     # the first fits one trip of ONE workgroup; the second does not


def f_sb(shape):
    return noise(shape, 300 + sum(shape)), 0.1


def f_all():
    return smoothed(noise((14, 12, 10, 33), 107), 2), 0.3        # (small enough for the oracle to take a second)


def f_all_other():
    return smoothed(noise((11, 9, 10, 40), 108), 2), 0.1


def cond_qcap(env):
    A, v = f_qcap()
    words = word_counts(active_cells(A, v))
    assert len(words) == 512
    fl = queue_flushes(words, queue_ipb(env, len(words)))
    # a wave's two steps together exceed the LDS queue, its words do not exceed the word table: the CX4_QCAP side alone
    assert fl and all(why == ["Q"] for why in fl.values())
    assert any(int(words[64 * w:64 * w + 64].sum() + words[256 + 64 * w:256 + 64 * w + 64].sum()) > CX4_QCAP for w in range(4))


def cond_wcap(env):
    A, v = f_wcap()
    words = word_counts(active_cells(A, v))
    assert len(words) >= 768 and A.shape[3] == 3
    fl = queue_flushes(words, queue_ipb(env, len(words)))
    assert fl and all(set(why) == {"W"} for why in fl.values())
    w = sorted(fl)[0][1]
    mine = np.concatenate([words[64 * w + 256 * s:64 * w + 256 * s + 64] for s in range(3)])
    assert int((mine > 0).sum()) > CX4_WCAP and int(mine.sum()) <= CX4_QCAP


def cond_both_512(env):
    A, v = f_both()
    assert A.shape[3] % 32 == 1                      # rows of 3 words, the last holds one lattice point (and a lane's `edge` bit)
    fl = flushes_of(A, v, env)
    assert len(set(blk for blk, _ in fl)) >= 2       # at least two workgroups each hold a flushing wave
    words = word_counts(active_cells(A, v))
    nblocks = (len(words) + 511) // 512
    assert len(fl) < 4 * nblocks                     # ... next to waves that reach their final flush without one


def cond_both_1024(env):
    fl = flushes_of(*f_both(), env)
    sides = set(s for why in fl.values() for s in why)
    assert "Q" in sides and any("W" in s for s in sides)       # both sides of the condition in one field


def cond_cells(env):
    A, v = f_cells()
    assert int(active_cells(A, v).sum()) > 4 * 512
    assert int(active_cells(A, v).sum()) > cells_wgs(env, A) * 512       # a second trip of the grid-stride loop


def cond_tets(env):
    seen = set()
    for shape, want_rounds in TETS_SHAPES:
        A, v = f_tets(shape)
        nrounds, nfull, nhalf = tets_rounds(env, A, v)
        assert nrounds == want_rounds
        if nrounds >= 5:
            assert nfull > 0                         # whole rounds (part == 0) ...
            seen.add(nrounds % 4)
            assert nhalf == nrounds % 4
        else:
            assert nfull == 0 and nhalf == nrounds   # ... and the field that runs as halves only
    assert seen >= {0, 1, 3}


def cond_sb(env):
    for shape in SB_ROW_SHAPES:
        kernel, trips = signbits_trips(env, f_sb(shape)[0])
        assert kernel == "rows" and trips >= 2
    assert (5 * 3 * 3 * 2) % 8 != 0                  # (5, 3, 3, 70): the last group of 8 chunks is clamped
    for shape, want in zip(SB_FLAT_SHAPES, (1, 2)):
        kernel, trips = signbits_trips(env, f_sb(shape)[0])
        assert kernel == "flat" and (trips >= 2) == (want >= 2)


def cond_sb_rows(env):
    for shape in SB_FLAT_SHAPES:
        kernel, trips = signbits_trips(env, f_sb(shape)[0])
        assert kernel == "rows" and trips >= 2


def cond_all(env):
    A, v = f_all()
    sides = set(s for why in flushes_of(A, v, env).values() for s in why)
    assert sides >= {"Q", "W", "QW"}
    assert int(active_cells(A, v).sum()) > cells_wgs(env, A) * 512
    nrounds, nfull, nhalf = tets_rounds(env, A, v)
    assert nfull > 0 and nhalf > 0
    assert signbits_trips(env, A) == ("rows", 27)    # n3 = 33: one chunk per row (the kernel's nchunk == 1 branch), 1680 rows


def run_fields(fields):
    return sum(check_both(A, v) for A, v in fields)


def run_sb(out):
    import torch
    from contourist_amd import _ffi
    n = run_fields([f_sb(s) for s in SB_ROW_SHAPES + SB_FLAT_SHAPES])
    saved = {}
    ctx = _ffi.Context(0)
    try:
        for shape in SB_FLAT_SHAPES:
            A, v = f_sb(shape)
            if os.environ.get("CX4_SB_ROWS") != "1":
                dev = torch.from_numpy(A).to("cuda:0").contiguous()
                assert dev.data_ptr() % 16 == 0      # or the flat kernel is not the one that ran
            else:
                dev = None
            for diagonal, mode in MODES:
                _, ch = check_ctx(ctx, A, v, mode, adopt=dev)
                for i, part in enumerate(ch):
                    saved["%s_%s_%d" % ("x".join(map(str, shape)), diagonal, i)] = part
    finally:
        ctx.close()
    if out:
        np.savez(out, **saved)
    return n


def run_all(out):
    from contourist_amd import _ffi
    A, v = f_all()
    B, vb = f_all_other()
    n = 0
    ctx = _ffi.Context(0)
    try:
        for diagonal, mode in MODES:
            # twice on one context, the second time after another shape: buffers that grew and the hash table are used again
            n += check_ctx(ctx, A, v, mode, key="all")[0]["n_tetrahedra"]
            check_ctx(ctx, B, vb, mode, key="other")
            check_ctx(ctx, A, v, mode, key="all")
        check_ctx(ctx, A, v, 1, key="all", use_async=True)           # cx_extract4d_async + cx_counts4d_get
        check_ctx(ctx, B, vb, 1, key="other", use_async=True)
    finally:
        ctx.close()
    return n


KNOB_CASES = {
    "flush_qcap": dict(env={"CX4_IPB": "512"}, cond=cond_qcap, run=lambda out: run_fields([f_qcap()])),
    "flush_wcap": dict(env={"CX4_IPB": "768"}, cond=cond_wcap, run=lambda out: run_fields([f_wcap()])),
    "flush_several_workgroups": dict(env={"CX4_IPB": "512"}, cond=cond_both_512, run=lambda out: run_fields([f_both()])),
    "flush_both_sides": dict(env={"CX4_IPB": "1024"}, cond=cond_both_1024, run=lambda out: run_fields([f_both()])),
    "cells_one_workgroup": dict(env={"CX4_CELLS_WGS": "1"}, cond=cond_cells, run=lambda out: run_fields([f_cells()])),
    "cells_three_workgroups": dict(env={"CX4_CELLS_WGS": "3"}, cond=cond_cells, run=lambda out: run_fields([f_cells()])),
    "tets_whole_rounds_and_halves": dict(env={"CX4_TETS_WGS": "1"}, cond=cond_tets,
                                         run=lambda out: run_fields([f_tets(s) for s, _ in TETS_SHAPES])),
    "signbits_grid_stride": dict(env={"CX4_SB_BLOCKS": "1"}, cond=cond_sb, run=run_sb),
    "signbits_grid_stride_rows": dict(env={"CX4_SB_BLOCKS": "1", "CX4_SB_ROWS": "1"}, cond=cond_sb_rows, run=run_sb),
    "all_knobs_small": dict(env={"CX4_IPB": "1024", "CX4_CELLS_WGS": "2", "CX4_TETS_WGS": "3", "CX4_SB_BLOCKS": "2"}, cond=cond_all,
                            run=run_all),
}


def case_env(name):
    return dict(KNOB_CASES[name]["env"], CX_DEBUG="1")


def run_knob_case(name, out=None):
    "in the child process: the knobs are those of the case, the input reaches the branch, the meshes are the oracle's"
    case = KNOB_CASES[name]
    for k, val in case_env(name).items():
        assert os.environ.get(k) == val, (k, os.environ.get(k))
    case["cond"](dict(os.environ))
    n = case["run"](out)
    print("MARCH4D_PATHS_OK", name, n, flush=True)


_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import test_gpu_march4d_paths as T
T.run_knob_case({name!r}, {out!r})
"""


def run_child(name, out=None):
    KNOB_CASES[name]["cond"](case_env(name))         # on the CPU, before any GPU call
    env = dict((k, val) for k, val in os.environ.items() if not k.startswith("CX4_"))
    env.update(case_env(name))
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("MARCH4D_PATHS_OK " + name + " ")]
    assert line, r.stdout[-2000:]
    assert int(line[0].split()[2]) > 0               # tetrahedra were compared


@pytest.mark.parametrize("name", [n for n in KNOB_CASES if not n.startswith("signbits")])
def test_branch_under_knobs(name):
    run_child(name)


def test_signbits_grid_stride_flat_and_rows_give_the_same_mesh(tmp_path):
    """CX4_SB_BLOCKS=1: second trips of both sign-bitmap kernels (rows: two and ten chunks per row, groups of 8 chunks that span rows,
    a clamped last group; flat: on an adopted device array whose 16-byte alignment is asserted).  The issue's flat shape (6, 5, 4, 64)
    is 1 920 quads and fits ONE trip of one workgroup (2 048 quads), so (7, 5, 5, 64) stands next to it.  Then the row kernel on the
    flat shapes (CX4_SB_ROWS=1): the same mesh as the flat kernel's, bit for bit, in canonical order."""
    flat, rows = str(tmp_path / "flat.npz"), str(tmp_path / "rows.npz")
    run_child("signbits_grid_stride", flat)
    run_child("signbits_grid_stride_rows", rows)
    F, R = np.load(flat), np.load(rows)
    assert sorted(F.files) == sorted(R.files) and len(F.files) == 3 * 2 * len(SB_FLAT_SHAPES)
    for k in F.files:
        assert F[k].dtype == R[k].dtype and F[k].shape == R[k].shape and F[k].tobytes() == R[k].tobytes(), k
        assert len(F[k]) > 0


# ---- without knobs -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx4():
    from contourist_amd import _ffi
    c = _ffi.Context(0)
    yield c
    c.close()


N_FUZZ = 48
N3_CHOICES = (2, 3, 31, 32, 33, 63, 64, 65, 96, 129)
ORIGIN_MIN = -1024                    # the lowest component cx_set_origin4d accepts
INT32_MAX = 2 ** 31 - 1               # the kernels hash lattice coordinates as 32-bit ints; the oracle takes int64


def fuzz_case(case):
    """case -> (A, isovalue, diag_mode, origin): a fixed slice of tools/fuzz_gpu4d.py.  What the CPU-side assertions below count is
    dealt by the case number (quantised: every third; isovalue: case % 5; origin kind: (case // 3) % 3; split: case % 2), the rest
    is drawn from np.random.RandomState(4242 + case)."""
    rng = np.random.RandomState(4242 + case)
    kind = rng.randint(0, 3)
    if kind == 0:
        shape = tuple(int(x) for x in rng.randint(2, 9, size=4))
    elif kind == 1:
        shape = (int(rng.randint(2, 12)), int(rng.randint(2, 12)), int(rng.randint(2, 12)), int(rng.choice(N3_CHOICES)))
    else:
        shape = (int(rng.randint(6, 20)), int(rng.randint(6, 20)), int(rng.randint(6, 20)), int(rng.randint(4, 24)))
    A = smoothed(rng.standard_normal(shape), int(rng.randint(0, 5)))
    if case % 3 == 0:
        A = quarters(A)
    v = (0.0, -0.0, 0.25, -0.5, float(np.float32(rng.uniform(-1.0, 1.0))))[case % 5]
    diag_mode = 1 - case % 2
    okind = (case // 3) % 3
    if okind == 0:
        origin = (0, 0, 0, 0)
    elif okind == 1:
        origin = tuple(int(x) for x in rng.randint(0, 51, size=4))
        if case == 4:     # as large as the kernels' 32-bit coordinates go: the last lattice point of axes 0 and 3 is INT32_MAX
            origin = (INT32_MAX - (shape[0] - 1), origin[1], 0, INT32_MAX - (shape[3] - 1))
    else:
        o = [int(x) for x in rng.randint(-3, 6, size=4)]
        o[(case // 9) % 4] = -1                                   # hash(-1) == -2, on each axis in turn
        if case == 8:
            o[(case // 9 + 1) % 4] = ORIGIN_MIN
        origin = tuple(o)
    return A, v, diag_mode, origin


def fuzz_slice_conditions():
    "conditions on the 48 inputs (CPU only; tests/test_march4d_paths_inputs.py runs them without a GPU as well)"
    both_zeros = nonzero_cpython = 0
    kinds = set()
    minus_one_axes = set()
    for case in range(N_FUZZ):
        A, v, diag_mode, origin = fuzz_case(case)
        if v == 0.0 and np.any((A == 0) & np.signbit(A)) and np.any((A == 0) & ~np.signbit(A)):
            both_zeros += 1
            kinds.add(bool(np.signbit(v)))
        nonzero_cpython += bool(diag_mode == 1 and any(origin))
        if diag_mode == 1:
            minus_one_axes |= set(d for d in range(4) if origin[d] == -1)
    assert both_zeros >= 6 and kinds == {False, True}              # zeros of either sign at isovalue 0.0 and at -0.0
    assert nonzero_cpython >= 10
    assert minus_one_axes == {0, 1, 2, 3}
    assert ORIGIN_MIN in fuzz_case(8)[3] and fuzz_case(8)[2] == 1
    A, _, mode, origin = fuzz_case(4)
    assert mode == 1 and origin[0] + A.shape[0] - 1 == INT32_MAX and origin[3] + A.shape[3] - 1 == INT32_MAX


def test_fuzz_slice_holds_what_it_is_for():
    fuzz_slice_conditions()


@pytest.mark.parametrize("case", range(N_FUZZ))
def test_fuzz_slice(ctx4, case):
    A, v, diag_mode, origin = fuzz_case(case)
    check_ctx(ctx4, A, v, diag_mode, origin)


def test_origin_beyond_32_bit_coordinates_is_refused(ctx4):
    """the oracle (and CPython) order sets of lattice points with coordinates of any size; the kernels hash them as 32-bit ints.  An origin
    that puts a lattice point beyond 2^31 - 1 is refused for the CPython split instead of silently ordered by other hashes; the canonical
    split does not hash and takes it; the context works on afterwards"""
    from contourist_amd import _ffi
    A = noise((4, 3, 5, 6), 77)
    for axis in range(4):
        o = [3, 2, 1, 0]
        o[axis] = INT32_MAX - (A.shape[axis] - 1) + 1
        ctx4.set_origin4d(*o)
        ctx4.upload_grid4d(A)
        with pytest.raises(_ffi.CxError):
            ctx4.extract4d(0.1, _ffi.CX_DIAG_CPYTHON310)
        check_ctx(ctx4, A, 0.1, 0, tuple(o))
    with pytest.raises(_ffi.CxError):
        ctx4.set_origin4d(0, ORIGIN_MIN - 1, 0, 0)
    check_ctx(ctx4, A, 0.1, 1, (0, 0, 0, INT32_MAX - (A.shape[3] - 1)))
    check_ctx(ctx4, A, 0.1, 1)


@pytest.mark.parametrize("shape", [(5, 4, 6, 7), (3, 4, 2, 64)])
def test_constant_fields(ctx4, shape):
    "all above, all below and all EQUAL to the isovalue (f == v is high): nothing to extract, and the context goes on working"
    from contourist_amd import _ffi
    A = np.full(shape, 1.0, dtype=np.float32)
    for v in (0.5, 2.0, 1.0):
        for flags in (_ffi.CX_DIAG_CPYTHON310, _ffi.CX_DIAG_CANONICAL):
            ctx4.upload_grid4d(A)
            c = ctx4.extract4d(v, flags)
            assert c == dict(n_cells=0, n_vertices=0, n_tetrahedra=0, n_border_voxels=0)
            verts, keys, tets = ctx4.download_level0_4d(c)
            assert len(verts) == 0 and len(keys) == 0 and len(tets) == 0
        for mode in (1, 0):
            check_ctx(ctx4, A, v, mode)                           # the oracle agrees that there is nothing
    B = noise(shape, 5)
    c, _ = check_ctx(ctx4, B, 0.1, 1)
    assert c["n_tetrahedra"] > 0
    Z = np.zeros(shape, dtype=np.float32)
    Z[::2] = -0.0
    for v in (0.0, -0.0):
        check_ctx(ctx4, Z, v, 1)                                  # zeros of both signs and nothing else: equal to either isovalue


def test_relative_tolerance_4d():
    """the pair test_tolerances_4d lacks (3-D: test_values_equal_to_isovalue_and_tolerances): samples within the reference's RELATIVE
    tolerance of an isovalue of 100, and an isovalue that is not an fp32 number (P.vhi + P.vlo, the double fall-back)"""
    rng = np.random.RandomState(9)
    C = (100.0 + rng.standard_normal((6, 5, 6, 7)) * 1.5e-3).astype(np.float32)
    for v in (100.0, 100.0007):
        assert check_both(C, v) > 0


# ---- the exact set order, on purpose ---------------------------------------------------------------------------------------------
def set_order_cases():
    ep, bp = setorder4d_cases.selected(*setorder4d_cases.BOX_POSITIVE)
    en, bn = setorder4d_cases.selected(*setorder4d_cases.BOX_NEGATIVE, want=2, negative_only=True)
    return [("exact", c) for c in ep] + [("boundary", c) for c in bp] + [("exact_negative", c) for c in en[:1]] + \
           [("boundary_negative", c) for c in bn[:1]]


def set_order_field(case, n, pos):
    """3 x 3 x 3 x 3 samples: the hyper-voxel at array position `pos` is low (-1) exactly at the case's 2-set and high (+1) at its other
    corners, seeded noise elsewhere (no sample is 0)"""
    A = np.random.RandomState(900 + n).standard_normal((3, 3, 3, 3)).astype(np.float32)
    A[A == 0] = 0.5
    for c in range(16):
        at = tuple(int(p + o) for p, o in zip(pos, setorder4d_cases.corner_offsets(c)))
        A[at] = -1.0 if c in case["corners2"] else 1.0
    return A


@pytest.mark.parametrize("n", range(18))
def test_exact_and_boundary_set_orders(ctx4, n):
    """sets whose members are still on a used slot after the six slots of their probe codes (cx_pent_perm_exact) and sets the LAST field
    decides: the hyper-voxel sits at the case's lattice coordinates through the origin; once with the 2-set low, once negated (the 3-set
    low), CPython split.  (A scratch build whose cx_pent_perm_exact returns permutation 0 fails 8 of the 9 exact cases here -- the ninth
    orders its sets as setorder4d_cases.SAME_AS_UNORDERED -- and one boundary case whose hyper-voxel holds another pentatope on the
    exact path; it also fails 16 of the 24 CPython-split cases of the fuzz slice: noise meets the exact path all the time.)"""
    cases = set_order_cases()
    assert len(cases) == 18
    kind, case = cases[n]
    pos = ((n >> 3) & 1, (n >> 2) & 1, (n >> 1) & 1, n & 1)         # each of the 16 hyper-voxels of the array in turn
    origin = tuple(c - p for c, p in zip(case["cell"], pos))
    A = set_order_field(case, n, pos)
    low = A[tuple(slice(p, p + 2) for p in pos)] < 0
    assert int(low.sum()) == 2
    assert kind.startswith("exact") == (max(case["reprobes"]) >= setorder4d_cases.PROBE_FIELDS)
    assert ("negative" in kind) == (min(case["cell"]) < 0)
    for B in (A, -A):
        c, _ = check_ctx(ctx4, B, 0.0, 1, origin)
        assert c["n_tetrahedra"] > 0
