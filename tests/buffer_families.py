"""The inputs, parameters and CPU references of the device-buffer families of tests/test_gpu_buffers.py that came after cx_buf: the
same arrays go to the device there and to the numpy restatements here (tests/test_buffer_families_host.py runs every reference once and
asserts that no case is trivial).  Importable without a GPU.  The references are taken at size small only: the restatements are brute
force and too slow for 64^3 in a test."""
import numpy as np

import distance_ref
import filter_ref
import label_ref
import levels_ref
import rank_ref
import recon_ref
import resample_ref
from test_gpu_typed_grid import _quantise

SHAPES3 = {"small": (29, 23, 67), "mid": (37, 41, 52), "large": (64, 64, 64)}   # those of test_exact_capacities
OPERATIONS = ("filter", "distance", "label", "resample", "rank", "reconstruct")


def _field3(size):
    shape = SHAPES3[size]
    rng = np.random.RandomState(11)
    g0, g1, g2 = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (np.sin(3.1 * g0 + 0.4) * np.cos(2.7 * g1) + 0.8 * np.sin(3.9 * g2 + 1.0) + 0.05 * rng.standard_normal(shape)).astype(np.float32)


def second_field(size):
    "B: a second smooth field of the shape of _field3(size), other phases and another seed"
    shape = SHAPES3[size]
    rng = np.random.RandomState(29)
    g0, g1, g2 = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    return (np.cos(2.3 * g0 - 0.7) * np.sin(3.3 * g2 + 0.2) + 0.7 * np.cos(4.1 * g1 + 0.5) + 0.05 * rng.standard_normal(shape)).astype(np.float32)


# the isovalue of a quantised copy: a value of the type that some samples equal (the host test asserts it)
TYPED_VALUES = {"uint8": 131.0, "int16": 1000.0}


def quantised(size, name):
    "_field3(size) rounded into the range of uint8 or int16"
    return _quantise(_field3(size), name)[0]


# ---- parameters: chosen so that no case is trivial (tests/test_buffer_families_host.py) ---------------------------------------------------
def _taps(seed):
    w = np.random.RandomState(seed).uniform(0.1, 1.0, size=3)
    return ((w / w.sum()).astype(np.float32), 1, 1)


FILTER_AXES = [_taps(0), _taps(1), _taps(2)]                 # all three axes: both kernels
FILTER_AXES_BOUND = [(None, 0, 1), _taps(3), _taps(4)]       # axis 0 left alone: one kernel
FILTER_MODE = "reflect"
DISTANCE_VALUE, DISTANCE_RADIUS2 = 0.1, 6.0
LABEL_VALUE = 0.9                                            # the caps of the field and specks of its noise around them
LABEL_CONNECTIVITIES = (1, 3)                                # host samples, the bound grid
RESAMPLE_ZOOM = (np.diag([1.25, 0.8, 1.1]), np.array([-2.5, 1.5, -3.0]))      # axis aligned: the table kernel
RESAMPLE_MODE, RESAMPLE_CVAL = "constant", -0.25
RANK_GENERAL = dict(size=3, rank=13, mode="reflect")                          # the median of 27
RANK_EXTREME = dict(size=(3, 3, 3), rank=26, mode="nearest")                  # the maximum of a full box: the separable kernel
RECON_SHIFT_H = 0.3
RECON_CONNECTIVITY = 1


def resample_turn(shape):
    "30 degrees about axis 0 through the centre, the output of the input's shape: the general kernel, corners outside"
    return resample_ref.about_centre(resample_ref.rotation(0, 30.0), shape, shape)


def keep_pattern(k):
    "K + 1 flags with both values among the labels and the unlabelled samples kept (that of tests/test_gpu_label.py)"
    return (np.arange(k + 1) % 3 != 1).astype(np.uint8)


def recon_marker(size, name="float32"):
    "a host marker below the mask _field3 (quantised(size, name)) on most samples and above it on some (those are clamped)"
    A, B = _field3(size), second_field(size)
    if name == "float32":
        return (A - 0.4 * np.abs(B) + np.where(B > 1.2, 0.6, 0.0)).astype(np.float32)
    Q = quantised(size, name).astype(np.int64)
    info = np.iinfo(np.dtype(name))
    return np.clip(Q - np.rint(40 * np.abs(B)).astype(np.int64) + np.where(B > 1.2, 60, 0), info.min, info.max).astype(name)


# ---- what a family's first downloads must be at size small, in the family's order -----------------------------------------------------------
def filter_expected(size="small"):
    return [filter_ref.filter3d(_field3(size), FILTER_AXES, FILTER_MODE)]


def distance_expected(size="small"):
    A = _field3(size)
    parts = distance_ref.both(A, DISTANCE_VALUE)
    return [distance_ref.distance(A, DISTANCE_VALUE, "signed", parts=parts), distance_ref.mask(A, DISTANCE_VALUE, "below", DISTANCE_RADIUS2, parts=parts)]


def label_expected(size="small"):
    "labels, records (as bytes' worth: the structured array), the mask of keep_pattern"
    A = _field3(size)
    labels, k = label_ref.label(A, LABEL_VALUE, "high", LABEL_CONNECTIVITIES[0])
    return [labels, label_ref.records(labels, k), label_ref.select(labels, keep_pattern(k))[0]]


def resample_expected(size="small"):
    A, U = _field3(size), quantised(size, "uint8")
    M, off = RESAMPLE_ZOOM
    Mt, offt = resample_turn(A.shape)
    return [resample_ref.resample(A, M, off, A.shape, 1, RESAMPLE_MODE, RESAMPLE_CVAL)[0],
            resample_ref.resample(U, Mt, offt, A.shape, 0, RESAMPLE_MODE, 7)[0]]


def resample_outside(size="small"):
    A = _field3(size)
    M, off = RESAMPLE_ZOOM
    Mt, offt = resample_turn(A.shape)
    return [resample_ref.resample(A, M, off, A.shape, 1, RESAMPLE_MODE, RESAMPLE_CVAL)[1],
            resample_ref.resample(quantised(size, "uint8"), Mt, offt, A.shape, 0, RESAMPLE_MODE, 7)[1]]


def rank_expected(size="small"):
    A, Q = _field3(size), quantised(size, "int16")
    g, e = RANK_GENERAL, RANK_EXTREME
    return [rank_ref.rank_filter(A, g["rank"], g["size"], None, None, g["mode"]), rank_ref.rank_filter(Q, e["rank"], e["size"], None, None, e["mode"])]


def recon_expected(size="small", stats=False):
    "shift on float32, step on uint8, a host marker on float32 -> the results (stats: (n_changed, n_clamped) of each instead)"
    A, U = _field3(size), quantised(size, "uint8")
    runs = [recon_ref.reconstruct(A, "shift", h=RECON_SHIFT_H, connectivity=RECON_CONNECTIVITY),
            recon_ref.reconstruct(U, "step", connectivity=RECON_CONNECTIVITY),
            recon_ref.reconstruct(A, recon_marker(size), connectivity=RECON_CONNECTIVITY)]
    return [r[1:] for r in runs] if stats else [r[0] for r in runs]


def pick_expected(size="small"):
    "the order statistics of the bound grid and of host samples of another length, the spectrum of the bound grid"
    A, other = _field3(size), pick_samples()
    return [levels_ref.select(A, pick_ranks(A.size))[0], levels_ref.select(other, pick_ranks(other.size))[0]] + \
        [levels_ref.spectrum(A, PICK_VALUES)[k] for k in levels_ref.KEYS]


PICK_VALUES = [-0.6, -0.3, 0.1, 0.5, 0.9]


def pick_ranks(n):
    return [0, n // 7, n // 2, n - 2, n - 1]


def pick_samples():
    "host samples whose length is no grid's"
    return np.random.RandomState(31).standard_normal(70001).astype(np.float32)


EXPECTED = {"filter": filter_expected, "distance": distance_expected, "label": label_expected, "resample": resample_expected,
            "rank": rank_expected, "reconstruct": recon_expected, "pick": pick_expected}


# ---- the chains: the result of call k is the samples of call k + 1, four calls ---------------------------------------------------------------
CHAIN_CALLS = 4


def chain_step(op, S, call):
    """call number `call` (from 0) of the chain of `op` on the samples S -> the list of its downloads, the last of them the samples of
    the next call.  The device side of tests/test_gpu_buffers.py makes the same calls with the same parameters."""
    if op == "filter":
        return [filter_ref.filter3d(S, FILTER_AXES, FILTER_MODE)]
    if op == "distance":
        return [distance_ref.distance(S, chain_distance_value(call), "signed")]
    if op == "label":
        labels, k = label_ref.label(S, chain_label_value(call), "high", LABEL_CONNECTIVITIES[0])
        return [labels, label_ref.select(labels, chain_keep(k))[0]]
    if op == "resample":
        M, off = RESAMPLE_ZOOM
        return [resample_ref.resample(S, M, off, S.shape, 1, RESAMPLE_MODE, RESAMPLE_CVAL)[0]]
    if op == "rank":
        g = RANK_GENERAL
        return [rank_ref.rank_filter(S, g["rank"], g["size"], None, None, g["mode"])]
    assert op == "reconstruct"
    return [recon_ref.reconstruct(S, "shift", h=RECON_SHIFT_H, connectivity=RECON_CONNECTIVITY)[0]]


def chain_distance_value(call):
    "the field's own threshold, then the samples of the distance field nearer than 1.5 to the other side"
    return DISTANCE_VALUE if call == 0 else 1.5


def chain_label_value(call):
    "the field's own threshold, then the ones of the uint8 mask"
    return LABEL_VALUE if call == 0 else 0.5


def chain_keep(k):
    "keep_pattern without the unlabelled samples: every call keeps two components of three, 10 -> 6 -> 4 -> 2 at size small"
    keep = keep_pattern(k)
    keep[0] = 0
    return keep


def chain_expected(op, size="small"):
    "the downloads of every call of the chain, call by call; reconstruct: and of the call whose marker lies inside its mask's buffer"
    S, out = _field3(size), []
    for call in range(CHAIN_CALLS):
        out.append(chain_step(op, S, call))
        S = out[-1][-1]
    if op == "reconstruct":
        out.append([inside_expected(S)])
    return out


def inside_expected(S):
    """the call whose mask is planes 0 .. n - 2 of the pending result S and whose marker is planes 1 .. n - 1 of it.  By erosion: the
    chain's dilations took the domes off S, so a marker from below would rebuild the mask exactly; its basins are still there"""
    return recon_ref.reconstruct(np.ascontiguousarray(S[:-1]), np.ascontiguousarray(S[1:]), method="erosion", connectivity=RECON_CONNECTIVITY)[0]
