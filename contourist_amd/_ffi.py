"""ctypes binding of libcontourist_hip.so (C ABI: include/contourist_hip.h).

The HIP library is the product path: if it is missing or cannot be loaded this module raises --
there is no CPU fallback anywhere in `contourist_amd`.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libcontourist_hip.so")
if os.environ.get("CX_DEBUG") == "1" and os.environ.get("CX_LIB_PATH"):   # A/B builds of the tools (tools/variants.sh)
    LIB_PATH = os.environ["CX_LIB_PATH"]

CX_OK = 0
CX_ERR_INVALID = -1
CX_ERR_STATE = -4
CX_ERR_CAPACITY = -5
CX_ERR_UNSUPPORTED = -6
CX_DIAG_CANONICAL = 0
CX_DIAG_CPYTHON310 = 1
CX_KERNEL_GENERIC = 0x100
CX_KERNEL_STAGED = 0x200
CX_KERNEL_FUSED = 0x400
CX_KERNEL_TILED = 0x800


class cx_component(ctypes.Structure):
    "one record of cx_level1_components (include/contourist_hip.h): 128 bytes"
    _fields_ = [("triangles", ctypes.c_int64), ("vertices", ctypes.c_int64), ("area", ctypes.c_double), ("volume", ctypes.c_double),
                ("centroid", ctypes.c_double * 3), ("bbox_lo", ctypes.c_double * 3), ("bbox_hi", ctypes.c_double * 3),
                ("flipped", ctypes.c_int32), ("closed", ctypes.c_int32), ("first_triangle", ctypes.c_int64),
                ("reserved", ctypes.c_double * 1)]


# the same record as a numpy structured type (what Context.level1_components returns)
COMPONENT_DTYPE = np.dtype([("triangles", "<i8"), ("vertices", "<i8"), ("area", "<f8"), ("volume", "<f8"), ("centroid", "<f8", (3,)),
                            ("bbox_lo", "<f8", (3,)), ("bbox_hi", "<f8", (3,)), ("flipped", "<i4"), ("closed", "<i4"),
                            ("first_triangle", "<i8"), ("reserved", "<f8", (1,))])

class cx_topology(ctypes.Structure):
    "one record of cx_level1_topology (include/contourist_hip.h): 64 bytes"
    _fields_ = [("triangles", ctypes.c_int64), ("vertices", ctypes.c_int64), ("edges", ctypes.c_int64), ("boundary_edges", ctypes.c_int64),
                ("nonmanifold_edges", ctypes.c_int64), ("euler", ctypes.c_int64), ("boundary_loops", ctypes.c_int32), ("genus", ctypes.c_int32),
                ("nonsimple_loops", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class cx_loop(ctypes.Structure):
    "one record of cx_level1_boundary_loops: 16 bytes"
    _fields_ = [("component", ctypes.c_int32), ("simple", ctypes.c_int32), ("first", ctypes.c_uint32), ("count", ctypes.c_uint32)]


class cx_filter_axis(ctypes.Structure):
    "one axis of cx_grid_filter3d: 24 bytes"
    _fields_ = [("weights", ctypes.c_void_p), ("n_weights", ctypes.c_int32), ("origin", ctypes.c_int32), ("stride", ctypes.c_int32)]


FILTER_MODES = {"nearest": 0, "reflect": 1, "constant": 2}
DIST_SIDES = {"below": 0, "above": 1, "signed": 2}                  # CX_DIST_*
DIST_KINDS = {"squared": 0, "float32": 1, "mask": 2}                # CX_DIST_OUT_*
DIST_KIND_DTYPES = {0: np.float64, 1: np.float32, 2: np.uint8}
TOPOLOGY_DTYPE = np.dtype([("triangles", "<i8"), ("vertices", "<i8"), ("edges", "<i8"), ("boundary_edges", "<i8"), ("nonmanifold_edges", "<i8"),
                           ("euler", "<i8"), ("boundary_loops", "<i4"), ("genus", "<i4"), ("nonsimple_loops", "<i4"), ("reserved", "<i4")])
LOOP_DTYPE = np.dtype([("component", "<i4"), ("simple", "<i4"), ("first", "<u4"), ("count", "<u4")])
LABEL_SIDES = {"high": 0, "low": 1}                                 # CX_LABEL_*
RECON_METHODS = {"dilation": 0, "erosion": 1}                       # CX_RECON_DILATION / _EROSION
RECON_MARKERS = {"array": 0, "shift": 1, "step": 2, "rim": 3}       # CX_RECON_MARKER_*
RECON_OUTS = {"values": 0, "changed": 1}                            # CX_RECON_OUT_*
RECON_ALL_FACES = 63                                                # bit 0: i = 0, 1: i = n0-1, 2: j = 0, 3: j = n1-1, 4: k = 0, 5: k = n2-1
RECON_STATS = ("n_changed", "n_clamped", "rounds", "tile_visits")   # cx_recon_stats, four int64
WATERSHED_DIRECTIONS = {"rising": 0, "falling": 1}                  # CX_WATERSHED_RISING / _FALLING
WATERSHED_STATS = ("n_labelled", "n_unreached", "n_ignored", "n_markers", "rounds", "tile_visits", "jump_rounds")   # cx_watershed_stats, seven int64
# one record of cx_grid_label3d_measures (cx_label_component): 72 bytes
LABEL_COMPONENT_DTYPE = np.dtype([("voxels", "<i8"), ("first", "<i8"), ("sum", "<i8", (3,)), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)),
                                  ("rim", "<u4"), ("reserved", "<u4")])
assert LABEL_COMPONENT_DTYPE.itemsize == 72
# one record of cx_grid_regions3d (cx_region): the measures of cx_label_component, then the value fields; 128 bytes
REGION_DTYPE = np.dtype(LABEL_COMPONENT_DTYPE.descr + [("n_nan", "<i8"), ("min_at", "<i8"), ("max_at", "<i8"), ("vmin", "<f8"), ("vmax", "<f8"),
                                                       ("isum", "<i8"), ("vsum", "<f8")])
# one record of cx_grid_regions3d_contacts (cx_region_contact): 32 bytes
REGION_CONTACT_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("faces", "<i8", (3,))])
assert REGION_DTYPE.itemsize == 128 and REGION_CONTACT_DTYPE.itemsize == 32
CX_REGIONS_MAX_LABEL = 1 << 24

# every symbol include/contourist_hip.h declares (tests check the library exports all of them)
SYMBOLS = [
    "cx_ctx_create", "cx_ctx_destroy", "cx_last_error", "cx_set_stream", "cx_synchronize",
    "cx_grid_upload", "cx_grid_adopt_device", "cx_grid_upload_typed", "cx_grid_adopt_device_typed", "cx_grid_info", "cx_grid_shadow_f64", "cx_set_origin", "cx_reserve",
    "cx_extract3d", "cx_extract3d_async", "cx_counts_get", "cx_extract3d_levels", "cx_levels_select", "cx_level0_path", "cx_level0_download", "cx_level0_device_ptrs", "cx_level0_device_records", "cx_level0_download_records",
    "cx_postprocess3d", "cx_postprocess3d_ex", "cx_level0_points_f64", "cx_postprocess3d_mesh", "cx_select_seeded3d", "cx_select_seeded3d_ex", "cx_seeded_masks_download", "cx_set_reference_corner", "cx_level1_download", "cx_level1_device_ptrs", "cx_level1_download_keys", "cx_postprocess3d_shard_begin", "cx_postprocess3d_shard_boundary", "cx_postprocess3d_shard_candidates", "cx_postprocess3d_shard_finish", "cx_level1_write", "cx_surface_geometry",
    "cx_level0_normals", "cx_level0_normals_download", "cx_level1_normals", "cx_level1_normals_download", "cx_level0_sample_grid", "cx_level1_sample_grid",
    "cx_level0_curvature", "cx_level0_curvature_download", "cx_level1_curvature", "cx_level1_curvature_download",
    "cx_level1_components", "cx_level1_components_download", "cx_level1_component_labels", "cx_level1_component_labels_download", "cx_level1_keep_components",
    "cx_level1_topology", "cx_level1_topology_download", "cx_level1_boundary_loops", "cx_level1_boundary_loops_download",
    "cx_level1_simplify", "cx_level1_simplify_map", "cx_level1_simplify_map_download",
    "cx_level1_clip_plane", "cx_level1_clip_scalars", "cx_level1_clip_map", "cx_level1_clip_map_download", "cx_level1_clip_info",
    "cx_cap3d", "cx_cap3d_download", "cx_cap3d_info", "cx_postprocess3d_capped",
    "cx_samples_select", "cx_level_spectrum3d",
    "cx_grid_filter3d", "cx_grid_filter3d_result", "cx_grid_filter3d_bind",
    "cx_grid_distance3d", "cx_grid_distance3d_result", "cx_grid_distance3d_bind",
    "cx_grid_label3d", "cx_grid_label3d_result", "cx_grid_label3d_measures", "cx_grid_label3d_select", "cx_grid_label3d_select_result", "cx_grid_label3d_bind",
    "cx_grid_resample3d", "cx_grid_resample3d_result", "cx_grid_resample3d_bind",
    "cx_grid_rank3d", "cx_grid_rank3d_result", "cx_grid_rank3d_bind",
    "cx_grid_reconstruct3d", "cx_grid_reconstruct3d_result", "cx_grid_reconstruct3d_bind",
    "cx_grid_watershed3d", "cx_grid_watershed3d_result",
    "cx_grid_regions3d", "cx_grid_regions3d_select", "cx_grid_regions3d_select_result", "cx_grid_regions3d_bind", "cx_grid_regions3d_map", "cx_grid_regions3d_contacts",
    "cx_grid4d_upload", "cx_grid4d_adopt_device", "cx_set_origin4d", "cx_extract4d", "cx_extract4d_async", "cx_counts4d_get", "cx_select_seeded4d", "cx_select_seeded4d_ex", "cx_seeded_mode", "cx_halo_exchange", "cx_rccl_unique_id", "cx_rccl_comm_init", "cx_rccl_comm_destroy", "cx_rccl_available", "cx_rccl_comm_share", "cx_slab_step", "cx_seeded4d_mask_download", "cx_level0_4d_download", "cx_postprocess4d", "cx_postprocess4d_points", "cx_level1_4d_download", "cx_morph_triangles", "cx_morph_download", "cx_morph_eval", "cx_morph_eval_download", "cx_morph_eval_many", "cx_morph_eval_many_download", "cx_morph_eval_many_device_ptrs", "cx_morph_eval_many_download_all",
    "cx_slab4d_begin", "cx_slab4d_append", "cx_slab4d_finish", "cx_slab4d_download_keys",
    "cx_contour2d_extract", "cx_contour2d_download",
    "cx_timing_enable", "cx_timing_read", "cx_measure_read_bandwidth", "cx_device_bytes", "cx_debug_stamps", "cx_version",
]
# sample types of a 3-D grid the kernels read as they are (CX_DTYPE_*): each converts to fp32 exactly.  Other types (int32, int64,
# float64) are not exact in fp32 and are widened on the host, as every type was before.
DTYPE_CODES = {"float32": 0, "uint8": 1, "int8": 2, "uint16": 3, "int16": 4, "float16": 5, "bfloat16": 6}
DTYPE_NAMES = {v: k for k, v in DTYPE_CODES.items()}


def dtype_code(dtype):
    """CX_DTYPE_* code of a numpy dtype, a torch dtype or a name ("int16", torch.bfloat16, np.uint8, ...); ValueError if the
    kernels do not read that type"""
    name = str(dtype)
    if name.startswith("torch."):
        name = name[len("torch."):]
    else:
        try:
            name = np.dtype(dtype).name
        except TypeError:
            pass
    if name not in DTYPE_CODES:
        raise ValueError("sample type %s is not one the 3-D kernels read (supported: %s)" % (dtype, ", ".join(DTYPE_CODES)))
    return DTYPE_CODES[name]


def native_array(array):
    """a numpy sample array of a type the kernels read, contiguous and in the machine's byte order (a big-endian '>i2' volume, as
    np.fromfile or FITS files give, is byte-swapped here; its raw bytes would be other numbers to the kernels)"""
    a = np.asarray(array)
    if not a.dtype.isnative:
        a = a.astype(a.dtype.newbyteorder("="))
    return np.ascontiguousarray(a)


def native_dtype(dtype):
    "True if a 3-D grid of this numpy / torch dtype is marched as it is (no fp32 copy)"
    try:
        dtype_code(dtype)
        return True
    except ValueError:
        return False


def locate_samples(samples, keep):
    """where the samples of a whole-volume operation are -> (pointer, CX_DTYPE_* code, on_device, shape).  samples: None = the bound
    grid; a 3-D numpy array of a type of DTYPE_CODES; (device pointer, dtype, shape) of contiguous samples on the device; or
    (numpy array, dtype, shape): host samples whose type is `dtype` whatever numpy calls their bytes (bfloat16 as uint16).  A host
    array is made contiguous and appended to the list `keep`, which has to outlive the call that reads the pointer."""
    if samples is None:
        return None, 0, 1, (0, 0, 0)
    if isinstance(samples, tuple):
        first, dtype, shape = samples
        host = np.ascontiguousarray(first) if isinstance(first, np.ndarray) else None
    else:
        host = native_array(samples)
        dtype, shape = host.dtype, host.shape
    if host is not None:
        keep.append(host)
    shape = tuple(int(n) for n in shape)
    assert len(shape) == 3, "3-D sample array expected"
    return ctypes.c_void_p(int(first) if host is None else host.ctypes.data), dtype_code(dtype), int(host is None), shape


def _download_array(shape, code):
    "an empty host array for a result of CX_DTYPE_* `code`: bfloat16, a type numpy has no name for, comes back as its uint16 bit patterns"
    name = DTYPE_NAMES.get(code, "float32")
    return np.empty([max(0, int(n)) for n in shape], dtype=np.uint16 if name == "bfloat16" else np.dtype(name))


CX_MESH_OF_THE_MARCH = 8     # cx_postprocess3d_mesh flags bit 3: the triangles are ones the march emitted (at most two per edge before merges)
CX_SIMPLIFY_NO_CLEAN = 1
CX_SIMPLIFY_ACROSS_COMPONENTS = 2
CX_SIMPLIFY_COUNT_ONLY = 4
CX_SIMPLIFY_NORMALS = 8
SIMPLIFY_KEYS = ("n_vertices", "n_triangles", "n_components", "n_clusters", "cell", "clamped")
CX_CLIP_NO_CLEAN = 1
CX_CLIP_KEEP_BELOW = 2
CX_CLIP_NORMALS = 4
CLIP_KEYS = ("n_vertices", "n_triangles", "n_components", "n_cut_vertices", "n_cut_triangles", "n_nonfinite", "n_on_cut")
CX_CAP_BELOW = 1
CX_CAP_ALL_FACES = 63
CAP_FACES = ("-x", "+x", "-y", "+y", "-z", "+z")      # bit 0: i = 0, bit 1: i = n0-1, bit 2: j = 0, ...
CAP_KEYS = ("n_lattice_vertices", "n_cap_triangles", "n_missing_crossings", "n_rim_crossings")
SPECTRUM_KEYS = ("n_cells", "n_vertices", "n_triangles", "n_near")


def cap_faces_mask(faces):
    """'all', a 6-bit mask, or a list of the names "-x", "+x", "-y", "+y", "-z", "+z" -> the mask of cx_cap3d"""
    if isinstance(faces, str):
        if faces == "all":
            return CX_CAP_ALL_FACES
        faces = [faces]
    if isinstance(faces, (int, np.integer)) and not isinstance(faces, bool):
        if int(faces) < 0 or int(faces) > CX_CAP_ALL_FACES:
            raise ValueError("a face mask has six bits, not %r" % (faces,))
        return int(faces)
    mask = 0
    for name in faces:
        if name not in CAP_FACES:
            raise ValueError("faces are named %s, not %r" % (", ".join(CAP_FACES), name))
        mask |= 1 << CAP_FACES.index(name)
    return mask


def cap_side_flags(side):
    if side not in ("above", "below"):
        raise ValueError("side is 'above' (cap where f >= value) or 'below' (where f < value), not %r" % (side,))
    return CX_CAP_BELOW if side == "below" else 0
CX2_ALL_CHAINS = 1
CX2_NO_DEDUPE = 2
CX2_SEARCH_SEEDS = 4


class CxCounts(ctypes.Structure):
    _fields_ = [("n_cells", ctypes.c_int64), ("n_vertices", ctypes.c_int64),
                ("n_triangles", ctypes.c_int64), ("n_border_voxels", ctypes.c_int64)]


class CxCounts2D(ctypes.Structure):
    _fields_ = [("n_points", ctypes.c_uint32), ("n_chains", ctypes.c_uint32), ("n_pairs", ctypes.c_uint32), ("n_levels", ctypes.c_uint32)]


CHAIN2D_DTYPE = np.dtype([("level", np.int32), ("closed", np.int32), ("first", np.uint32), ("count", np.uint32)])


class HipLibraryMissing(RuntimeError):
    pass


_lib = None


def _share_hip_runtime_with_torch():
    """One process must not hold two HIP runtimes.  A PyTorch-ROCm wheel ships its own libamdhip64.so and names it
    without the version, so the dynamic loader does not recognise ROCm's libamdhip64.so.7 (loaded for this
    library) as the same thing: torch.cuda then finds "no HIP GPUs".  If such a wheel is installed, load ITS
    runtime first -- this library's NEEDED libamdhip64.so.7 binds to it by soname -- whether or not torch gets
    imported later.  Without torch the ROCm copy on the library's RUNPATH is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(path):
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass   # best effort: the library itself still loads (against ROCm's runtime)


def load():
    """load (once) and type the shared library; raises HipLibraryMissing loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise HipLibraryMissing(
            "%s not found: build it with `python -m contourist_amd.build` (hipcc --offload-arch=gfx950). "
            "contourist_amd has no CPU fallback." % LIB_PATH)
    _share_hip_runtime_with_torch()
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, u32, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32, ctypes.c_double
    L.cx_version.restype = ctypes.c_char_p
    L.cx_version.argtypes = []
    L.cx_last_error.restype = ctypes.c_char_p
    L.cx_last_error.argtypes = [vp]
    sigs = {
        "cx_ctx_create": [ctypes.c_int, ctypes.POINTER(vp)],
        "cx_ctx_destroy": [vp],
        "cx_set_stream": [vp, vp],
        "cx_synchronize": [vp],
        "cx_grid_upload": [vp, vp, i64, i64, i64],
        "cx_grid_adopt_device": [vp, vp, i64, i64, i64],
        "cx_grid_upload_typed": [vp, vp, ctypes.c_int32, i64, i64, i64],
        "cx_grid_adopt_device_typed": [vp, vp, ctypes.c_int32, i64, i64, i64],
        "cx_grid_info": [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)],
        "cx_grid_shadow_f64": [vp, vp, i64, i64, i64],
        "cx_set_origin": [vp, i64, i64, i64],
        "cx_reserve": [vp, i64, i64, i64],
        "cx_extract3d": [vp, dbl, u32, ctypes.POINTER(CxCounts)],
        "cx_extract3d_async": [vp, dbl, u32],
        "cx_counts_get": [vp, ctypes.POINTER(CxCounts)],
        "cx_level0_path": [vp, ctypes.POINTER(ctypes.c_int)],
        "cx_extract3d_levels": [vp, vp, ctypes.c_int32, u32, vp],
        "cx_levels_select": [vp, ctypes.c_int32],
        "cx_level0_download": [vp, vp, vp],
        "cx_level0_device_ptrs": [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "cx_level0_device_records": [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "cx_level0_download_records": [vp, vp, vp],
        "cx_postprocess3d": [vp, u32, vp],
        "cx_postprocess3d_ex": [vp, u32, dbl, vp],
        "cx_level0_points_f64": [vp, vp],
        "cx_postprocess3d_mesh": [vp, vp, i64, vp, i64, vp, u32, dbl, vp],
        "cx_select_seeded3d": [vp, vp, i64, vp, vp],
        "cx_select_seeded3d_ex": [vp, vp, i64, vp, u32, vp],
        "cx_seeded_masks_download": [vp, vp, vp],
        "cx_set_reference_corner": [vp, i64, i64, i64],
        "cx_level1_download": [vp, vp, vp],
        "cx_level1_device_ptrs": [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(i64), ctypes.POINTER(i64)],
        "cx_level1_download_keys": [vp, vp],
        "cx_postprocess3d_shard_begin": [vp, u32, i64, i64, vp, vp, vp, vp],
        "cx_postprocess3d_shard_boundary": [vp, ctypes.c_int, vp, vp],
        "cx_postprocess3d_shard_candidates": [vp, vp, vp, vp, vp, vp, vp],
        "cx_postprocess3d_shard_finish": [vp, vp, vp, i64, vp],
        "cx_level1_write": [vp, ctypes.c_int, ctypes.c_char_p, vp, vp],
        "cx_surface_geometry": [vp, vp, ctypes.POINTER(i64), vp, ctypes.POINTER(i64), ctypes.c_int],
        "cx_level0_normals": [vp, vp, ctypes.POINTER(vp)],
        "cx_level0_normals_download": [vp, vp, vp],
        "cx_level1_normals": [vp, vp, ctypes.POINTER(vp)],
        "cx_level1_normals_download": [vp, vp, vp],
        "cx_level0_curvature": [vp, vp, ctypes.POINTER(vp)],
        "cx_level0_curvature_download": [vp, vp, vp],
        "cx_level1_curvature": [vp, vp, ctypes.POINTER(vp)],
        "cx_level1_curvature_download": [vp, vp, vp],
        "cx_level0_sample_grid": [vp, vp, ctypes.c_int32, ctypes.c_int, ctypes.POINTER(vp), vp],
        "cx_level1_sample_grid": [vp, vp, ctypes.c_int32, ctypes.c_int, ctypes.POINTER(vp), vp],
        "cx_level1_components": [vp, vp, ctypes.POINTER(i64), ctypes.POINTER(vp), vp],
        "cx_level1_components_download": [vp, vp, vp],
        "cx_level1_component_labels": [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "cx_level1_component_labels_download": [vp, vp, vp],
        "cx_level1_keep_components": [vp, vp, vp],
        "cx_level1_topology": [vp, ctypes.POINTER(i64), ctypes.POINTER(vp)],
        "cx_level1_topology_download": [vp, vp],
        "cx_level1_boundary_loops": [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "cx_level1_boundary_loops_download": [vp, vp, vp],
        "cx_level1_simplify": [vp, vp, ctypes.c_uint32, vp, vp],
        "cx_level1_simplify_map": [vp, ctypes.POINTER(vp)],
        "cx_level1_simplify_map_download": [vp, vp],
        "cx_level1_clip_plane": [vp, vp, ctypes.c_uint32, vp],
        "cx_level1_clip_scalars": [vp, vp, ctypes.c_int, ctypes.c_double, ctypes.c_uint32, vp],
        "cx_level1_clip_map": [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)],
        "cx_level1_clip_map_download": [vp, vp, vp],
        "cx_level1_clip_info": [vp, vp],
        "cx_cap3d": [vp, u32, u32, vp],
        "cx_cap3d_download": [vp, vp, vp],
        "cx_cap3d_info": [vp, vp],
        "cx_samples_select": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, vp, ctypes.c_int32, vp, ctypes.POINTER(i64)],
        "cx_level_spectrum3d": [vp, vp, ctypes.c_int32, vp, vp, vp, vp],
        "cx_postprocess3d_capped": [vp, u32, vp],
        "cx_grid_filter3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, vp, ctypes.c_int32, dbl, vp, vp, vp],
        "cx_grid_filter3d_result": [vp, ctypes.POINTER(vp), vp],
        "cx_grid_filter3d_bind": [vp],
        "cx_grid_distance3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, dbl, vp, ctypes.c_int32, ctypes.c_int32, dbl, vp, vp, vp],
        "cx_grid_distance3d_result": [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)],
        "cx_grid_distance3d_bind": [vp],
        "cx_grid_label3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, dbl, ctypes.c_int32, ctypes.c_int32, vp, vp, vp],
        "cx_grid_label3d_result": [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)],
        "cx_grid_label3d_measures": [vp, vp, i64],
        "cx_grid_label3d_select": [vp, vp, i64, vp, vp, vp],
        "cx_grid_label3d_select_result": [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_int64)],
        "cx_grid_label3d_bind": [vp],
        "cx_grid_resample3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, dbl, vp, vp, vp],
        "cx_grid_resample3d_result": [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)],
        "cx_grid_resample3d_bind": [vp],
        "cx_grid_rank3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, vp, vp, vp, ctypes.c_int32, ctypes.c_int32, dbl, vp, vp],
        "cx_grid_rank3d_result": [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_int32)],
        "cx_grid_rank3d_bind": [vp],
        "cx_grid_reconstruct3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, vp, ctypes.c_int32, dbl, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                  ctypes.c_int32, vp, vp, vp],
        "cx_grid_reconstruct3d_result": [vp, ctypes.POINTER(vp), vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)],
        "cx_grid_reconstruct3d_bind": [vp],
        "cx_grid_watershed3d": [vp, vp, ctypes.c_int32, ctypes.c_int, i64, i64, i64, vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp, vp],
        "cx_grid_watershed3d_result": [vp, ctypes.POINTER(vp), vp],
        "cx_grid_regions3d": [vp, vp, ctypes.c_int, i64, i64, i64, vp, ctypes.c_int32, ctypes.c_int, vp, i64, vp, vp],
        "cx_grid_regions3d_select": [vp, vp, ctypes.c_int, i64, i64, i64, vp, i64, vp, vp, ctypes.c_int32, vp, vp, vp, vp, vp],
        "cx_grid_regions3d_select_result": [vp, ctypes.POINTER(vp), vp, vp, ctypes.POINTER(ctypes.c_int64)],
        "cx_grid_regions3d_bind": [vp],
        "cx_grid_regions3d_map": [vp, vp, ctypes.c_int, i64, i64, i64, vp, i64, vp, vp],
        "cx_grid_regions3d_contacts": [vp, vp, ctypes.c_int, i64, i64, i64, vp, i64, vp],
        "cx_debug_stamps": [vp, i64, vp],
        "cx_grid4d_upload": [vp, vp, i64, i64, i64, i64],
        "cx_grid4d_adopt_device": [vp, vp, i64, i64, i64, i64],
        "cx_set_origin4d": [vp, i64, i64, i64, i64],
        "cx_extract4d": [vp, dbl, u32, ctypes.POINTER(CxCounts)],
        "cx_extract4d_async": [vp, dbl, u32],
        "cx_counts4d_get": [vp, ctypes.POINTER(CxCounts)],
        "cx_select_seeded4d": [vp, vp, i64, vp],
        "cx_select_seeded4d_ex": [vp, vp, i64, vp, ctypes.c_uint32, vp],
        "cx_seeded4d_mask_download": [vp, vp],
        "cx_seeded_mode": [vp, vp],
        "cx_halo_exchange": [vp, vp, ctypes.c_int, ctypes.c_int, vp, i64, i64],
        "cx_rccl_unique_id": [vp],
        "cx_rccl_comm_init": [vp, vp, ctypes.c_int, ctypes.c_int],
        "cx_rccl_comm_destroy": [vp],
        "cx_rccl_available": [],
        "cx_rccl_comm_share": [vp, vp],
        "cx_slab_step": [vp, vp, i64, i64, i64, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_uint32],
        "cx_level0_4d_download": [vp, vp, vp, vp],
        "cx_postprocess4d": [vp, ctypes.c_int32, vp],
        "cx_postprocess4d_points": [vp, ctypes.c_int32, vp, vp],
        "cx_level1_4d_download": [vp, vp, vp],
        "cx_morph_triangles": [vp, vp],
        "cx_morph_download": [vp, vp, vp, vp],
        "cx_morph_eval": [vp, dbl, vp],
        "cx_morph_eval_download": [vp, vp, vp],
        "cx_morph_eval_many": [vp, vp, ctypes.c_int32, vp],
        "cx_morph_eval_many_download": [vp, ctypes.c_int32, vp, vp],
        "cx_morph_eval_many_device_ptrs": [vp, ctypes.c_int32, vp, vp],
        "cx_morph_eval_many_download_all": [vp, vp, vp],
        "cx_slab4d_begin": [vp, vp],
        "cx_slab4d_append": [vp, i64, i64, vp],
        "cx_slab4d_finish": [vp, ctypes.c_int32, vp],
        "cx_slab4d_download_keys": [vp, vp],
        "cx_contour2d_extract": [vp, vp, ctypes.c_int, i64, i64, vp, ctypes.c_int32, vp, i64, u32, vp, ctypes.POINTER(CxCounts2D)],
        "cx_contour2d_download": [vp, vp, vp, vp],
        "cx_timing_enable": [vp, ctypes.c_int],
        "cx_timing_read": [vp, ctypes.POINTER(dbl), ctypes.POINTER(ctypes.c_int)],
        "cx_measure_read_bandwidth": [vp, vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(dbl)],
        "cx_device_bytes": [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.restype = ctypes.c_int
        fn.argtypes = args
    _lib = L
    return L


def device_bytes(handle=None):
    """(live bytes, hipMalloc calls so far) of the library's device buffers: of the context with this handle, or of the whole process"""
    live, allocations = ctypes.c_int64(), ctypes.c_int64()
    rc = load().cx_device_bytes(handle, ctypes.byref(live), ctypes.byref(allocations))
    if rc:
        raise CxError(rc, "cx_device_bytes")
    return live.value, allocations.value


class CxError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "contourist_hip error %d: %s" % (code, message))
        self.code = code


class Context(object):
    """One device + one HIP stream (cx_ctx).  Not thread safe."""

    def __init__(self, device=0, stream=None):
        self.lib = load()
        h = ctypes.c_void_p()
        rc = self.lib.cx_ctx_create(int(device), ctypes.byref(h))
        if rc != CX_OK:
            raise CxError(rc, "cx_ctx_create(device=%d) failed (no HIP device?)" % device)
        self.handle = h
        self.device = int(device)
        self._keep = None      # keeps an adopted tensor / uploaded array alive
        self.shape = None
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.cx_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != CX_OK:
            raise CxError(rc, self.lib.cx_last_error(self.handle).decode("utf-8", "replace"))

    def set_stream(self, stream):
        self._check(self.lib.cx_set_stream(self.handle, ctypes.c_void_p(int(stream) if stream else 0)))

    def synchronize(self):
        self._check(self.lib.cx_synchronize(self.handle))

    def upload_grid(self, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        assert a.ndim == 3, "3-D sample array expected"
        self._check(self.lib.cx_grid_upload(self.handle, a.ctypes.data, *a.shape))
        self.shape = tuple(int(n) for n in a.shape)
        self._keep = None

    def upload_grid_native(self, array):
        """the samples in their own type when the kernels read it (uint8, int8, uint16, int16, float16: n*sizeof(T) bytes on
        the device, no fp32 copy); any other type is widened to fp32 as upload_grid does"""
        a = np.asarray(array)
        assert a.ndim == 3, "3-D sample array expected"
        if not native_dtype(a.dtype) or dtype_code(a.dtype) == 0:
            return self.upload_grid(a)
        a = native_array(a)
        self._check(self.lib.cx_grid_upload_typed(self.handle, a.ctypes.data, dtype_code(a.dtype), *a.shape))
        self.shape = tuple(int(n) for n in a.shape)
        self._keep = None

    def adopt_device_grid(self, device_ptr, shape, keepalive=None, dtype="float32"):
        "samples already on the device (contiguous, of `dtype`: float32 or a type of DTYPE_CODES), not copied"
        assert len(shape) == 3
        code = dtype_code(dtype)
        if code == 0:
            self._check(self.lib.cx_grid_adopt_device(self.handle, ctypes.c_void_p(int(device_ptr)), *[int(n) for n in shape]))
        else:
            self._check(self.lib.cx_grid_adopt_device_typed(self.handle, ctypes.c_void_p(int(device_ptr)), code, *[int(n) for n in shape]))
        self.shape = tuple(int(n) for n in shape)
        self._keep = keepalive

    def grid_info(self):
        "dict(dtype=name of the bound grid's sample type, device_bytes=what the context holds for it: 0 for an adopted grid)"
        dt, nb = ctypes.c_int32(), ctypes.c_int64()
        self._check(self.lib.cx_grid_info(self.handle, ctypes.byref(dt), ctypes.byref(nb)))
        return dict(dtype=DTYPE_NAMES[int(dt.value)], device_bytes=int(nb.value))

    def shadow_grid_f64(self, array=None):
        """float64 originals of the bound samples (None drops them): Level 1 interpolates the crossings on these, as the
        reference does on the float64 values of its callable (tetrahedral.py:471-487)"""
        if array is None:
            self._check(self.lib.cx_grid_shadow_f64(self.handle, None, 0, 0, 0))
            return
        a = np.ascontiguousarray(array, dtype=np.float64)
        assert tuple(a.shape) == tuple(self.shape), (a.shape, self.shape)
        self._check(self.lib.cx_grid_shadow_f64(self.handle, a.ctypes.data, *a.shape))

    def set_origin(self, o0=0, o1=0, o2=0):
        self._check(self.lib.cx_set_origin(self.handle, int(o0), int(o1), int(o2)))

    def set_origin4d(self, o0=0, o1=0, o2=0, o3=0):
        "lattice coordinates of sample [0,0,0,0] in the reference's grid (negative: the array carries a rim of extra samples)"
        self._check(self.lib.cx_set_origin4d(self.handle, int(o0), int(o1), int(o2), int(o3)))

    def reserve(self, max_cells=0, max_vertices=0, max_triangles=0):
        self._check(self.lib.cx_reserve(self.handle, int(max_cells), int(max_vertices), int(max_triangles)))

    def extract3d(self, value, flags=CX_DIAG_CPYTHON310):
        c = CxCounts()
        self._check(self.lib.cx_extract3d(self.handle, float(value), int(flags), ctypes.byref(c)))
        return dict(n_cells=c.n_cells, n_vertices=c.n_vertices, n_triangles=c.n_triangles,
                    n_border_voxels=c.n_border_voxels)

    def extract3d_levels(self, values, flags=CX_DIAG_CPYTHON310):
        """all isovalues of `values` in one call (one pass over the samples for all of them) -> list of counts dicts;
        select_level(i) then makes level i the current extraction for download_level0 / postprocess3d / ..."""
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        out = (CxCounts * len(vals))()
        self._check(self.lib.cx_extract3d_levels(self.handle, vals.ctypes.data, len(vals), int(flags), ctypes.cast(out, ctypes.c_void_p)))
        return [dict(n_cells=c.n_cells, n_vertices=c.n_vertices, n_triangles=c.n_triangles, n_border_voxels=c.n_border_voxels) for c in out]

    def select_level(self, index):
        self._check(self.lib.cx_levels_select(self.handle, int(index)))

    def extract3d_async(self, value, flags=CX_DIAG_CPYTHON310):
        self._check(self.lib.cx_extract3d_async(self.handle, float(value), int(flags)))

    def counts(self):
        c = CxCounts()
        self._check(self.lib.cx_counts_get(self.handle, ctypes.byref(c)))
        return dict(n_cells=c.n_cells, n_vertices=c.n_vertices, n_triangles=c.n_triangles,
                    n_border_voxels=c.n_border_voxels)

    def download_level0(self, counts):
        """-> (xyz (V,3) float32 grid coordinates, edge ids (V,) uint32, triangles (T,3) int32)"""
        nv, nt = int(counts["n_vertices"]), int(counts["n_triangles"])
        verts = np.empty((nv, 4), dtype=np.float32)
        tris = np.empty((nt, 3), dtype=np.int32)
        self._check(self.lib.cx_level0_download(self.handle, verts.ctypes.data, tris.ctypes.data))
        keys = verts[:, 3].copy().view(np.uint32)
        return verts[:, :3].copy(), keys, tris

    def download_level0_records(self, counts):
        """-> (edge ids (V,) uint32, t (V,) float32: the crossing sits at q + t d on the lattice edge the id names, triangles (T,3) int32):
        the 8-byte records as the march leaves them (no expansion to coordinates)"""
        nv, nt = int(counts["n_vertices"]), int(counts["n_triangles"])
        recs = np.empty((nv, 2), dtype=np.uint32)
        tris = np.empty((nt, 3), dtype=np.int32)
        self._check(self.lib.cx_level0_download_records(self.handle, recs.ctypes.data, tris.ctypes.data))
        return recs[:, 0].copy(), recs[:, 1].copy().view(np.float32), tris

    def set_reference_corner(self, corner=(0, 0, 0)):
        self._check(self.lib.cx_set_reference_corner(self.handle, *[int(c) for c in corner]))

    def select_seeded(self, endpoints, voxel_range=None, all_in_range=False, parallel=False):
        """restrict the next post-passes to the components reached from `endpoints` (n x 2 x 3 lattice points);
        voxel_range = (lo[3], hi[3]) in_range box of the growth (default: the whole array);
        -> dict(seed_voxels, groups_kept, triangles_kept); groups_kept: the connected groups of surface voxels inside the box that
        are kept (a seed voxel outside the box is no group; with all_in_range: every group of the box)"""
        ep = np.ascontiguousarray(np.asarray(endpoints, dtype=np.int64).reshape(-1, 6), dtype=np.int32)
        out = np.zeros(4, dtype=np.int64)
        box = None
        if voxel_range is not None:
            box = np.ascontiguousarray(np.asarray(voxel_range, dtype=np.int64).reshape(6), dtype=np.int32)
        self._check(self.lib.cx_select_seeded3d_ex(self.handle, ep.ctypes.data, int(len(ep)),
                                                   box.ctypes.data if box is not None else None, (1 if all_in_range else 0) | (2 if parallel else 0), out.ctypes.data))
        return dict(seed_voxels=int(out[0]), groups_kept=int(out[1]), triangles_kept=int(out[2]))

    def seeded_masks(self, counts):
        "(triangle mask, vertex mask) of the last select_seeded as bool arrays (all True without a selection)"
        tk = np.empty(int(counts["n_triangles"]), dtype=np.uint8)
        vk = np.empty(int(counts["n_vertices"]), dtype=np.uint8)
        self._check(self.lib.cx_seeded_masks_download(self.handle, tk.ctypes.data, vk.ctypes.data))
        return tk.astype(bool), vk.astype(bool)

    def postprocess3d(self, flags=0, smooth=0.0):
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_postprocess3d_ex(self.handle, int(flags), float(smooth or 0.0), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_after_weld=int(out[2]),
                    n_after_tiny=int(out[3]), n_components=int(out[4]))

    def cap3d(self, faces="all", side="above"):
        """build the rim cap of the current extraction (cx_cap3d) -> dict of CAP_KEYS; faces: 'all', a mask or names of CAP_FACES"""
        out = np.zeros(4, dtype=np.int64)
        self._check(self.lib.cx_cap3d(self.handle, cap_faces_mask(faces), cap_side_flags(side), out.ctypes.data))
        return dict(zip(CAP_KEYS, (int(x) for x in out)))

    def download_cap(self, counts):
        """the raw cap -> (keys (C,) uint32 in ascending order: lattice points carry direction 0, triangles (K,3) int32 into the Level-0
        vertices followed by the cap vertices); counts: what cap3d returned"""
        keys = np.empty(int(counts["n_lattice_vertices"]) + int(counts["n_missing_crossings"]), dtype=np.uint32)
        tris = np.empty((int(counts["n_cap_triangles"]), 3), dtype=np.int32)
        self._check(self.lib.cx_cap3d_download(self.handle, keys.ctypes.data, tris.ctypes.data))
        return keys, tris

    def cap_info(self):
        "of the current cap: dict(ms, n_rim_records, table_slots, n_rim_points)"
        out = np.zeros(4, dtype=np.float64)
        self._check(self.lib.cx_cap3d_info(self.handle, out.ctypes.data))
        return dict(ms=float(out[0]), n_rim_records=int(out[1]), table_slots=int(out[2]), n_rim_points=int(out[3]))

    def postprocess3d_capped(self, flags=0):
        "Level 1 of the Level-0 mesh followed by the current cap (cap3d first) -> the same dict as postprocess3d"
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_postprocess3d_capped(self.handle, int(flags), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_after_weld=int(out[2]),
                    n_after_tiny=int(out[3]), n_components=int(out[4]))

    def samples_select(self, ranks, samples=None, dtype=None, n=None):
        """exact order statistics (cx_samples_select) -> (values float64 in the order of `ranks`, number of NaN samples).
        samples: None = the bound 3-D grid; a numpy array of a type of DTYPE_CODES (copied to the device); or a device pointer (int)
        with `dtype` and `n`"""
        rk = np.ascontiguousarray(ranks, dtype=np.int64).reshape(-1)
        out = np.empty(len(rk), dtype=np.float64)
        n_nan = ctypes.c_int64()
        if samples is None:
            ptr, code, on_device, count, keep = None, 0, 1, 0, None
        elif isinstance(samples, (int, np.integer)):
            ptr, code, on_device, count, keep = ctypes.c_void_p(int(samples)), dtype_code(dtype), 1, int(n), None
        else:
            keep = native_array(samples)
            ptr, code, on_device, count = ctypes.c_void_p(keep.ctypes.data), dtype_code(keep.dtype), 0, int(keep.size)
        self._check(self.lib.cx_samples_select(self.handle, ptr, code, on_device, count, rk.ctypes.data, len(rk), out.ctypes.data, ctypes.byref(n_nan)))
        return out, int(n_nan.value)

    def level_spectrum3d(self, values):
        """the size of the bound grid's isosurface at every one of `values` (cx_level_spectrum3d) -> dict of four int64 arrays in the
        order of `values`: n_cells, n_vertices, n_triangles, n_near"""
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        out = {k: np.zeros(len(vals), dtype=np.int64) for k in SPECTRUM_KEYS}
        self._check(self.lib.cx_level_spectrum3d(self.handle, vals.ctypes.data, len(vals), *[out[k].ctypes.data for k in SPECTRUM_KEYS]))
        return out

    def _bind_pending(self, result_fn, bind_fn):
        "the result that result_fn describes becomes the bound grid through bind_fn, an operation's cx_grid_*_bind"
        shape = result_fn()[0]
        self._check(bind_fn(self.handle))
        self.shape = shape
        self._keep = None

    def filter_grid(self, axes, mode="nearest", cval=0.0, samples=None, out=None, download=False):
        """separable filter with a stride per axis (cx_grid_filter3d) -> (shape of the result, the result).
        axes: three of (weights or None, origin, stride), for axis 0, 1, 2.  mode: a name of FILTER_MODES.
        samples: None = the bound 3-D grid; a 3-D numpy array of a type of DTYPE_CODES (copied to the device);
        (device pointer, dtype, shape) of contiguous samples on the device; or (numpy array, dtype, shape): host samples whose
        type is `dtype` whatever numpy calls their bytes.
        out: None = the result stays in the context (filter_result, bind_filtered); or a device pointer to room for the result.
        The result: a numpy array with download=True, else its device pointer (an int; the context's own buffer is valid until the
        next filter_grid or bind_filtered)."""
        assert len(axes) == 3
        recs, keep = (cx_filter_axis * 3)(), []
        for a, (weights, origin, stride) in enumerate(axes):
            w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            keep.append(w)
            recs[a].weights = None if w is None or not len(w) else w.ctypes.data
            recs[a].n_weights = 0 if w is None else len(w)
            recs[a].origin, recs[a].stride = int(origin), int(stride)
        ptr, code, on_device, shape = locate_samples(samples, keep)
        m = np.zeros(3, dtype=np.int64)
        if download:      # the shape first: it follows from the shape and the strides alone
            n = self.shape if samples is None else shape
            if n is None:
                raise CxError(CX_ERR_STATE, "filter_grid: no samples given and no grid bound")
            host_out = np.empty([-(-int(n[a]) // max(1, int(axes[a][2]))) for a in range(3)], dtype=np.float32)
        self._check(self.lib.cx_grid_filter3d(self.handle, ptr, code, on_device, shape[0], shape[1], shape[2], ctypes.cast(recs, ctypes.c_void_p),
                                              FILTER_MODES[mode], float(cval), ctypes.c_void_p(int(out)) if out else None,
                                              host_out.ctypes.data if download else None, m.ctypes.data))
        shape_out = tuple(int(x) for x in m)
        if download:
            assert host_out.shape == shape_out
            return shape_out, host_out
        return shape_out, (int(out) if out else self.filter_result()[1])

    def filter_result(self):
        "(shape, device pointer) of the result the last filter_grid left in the context (cx_grid_filter3d_result)"
        p, m = ctypes.c_void_p(), np.zeros(3, dtype=np.int64)
        self._check(self.lib.cx_grid_filter3d_result(self.handle, ctypes.byref(p), m.ctypes.data))
        return tuple(int(x) for x in m), int(p.value or 0)

    def bind_filtered(self):
        "the result the last filter_grid left in the context becomes the bound grid (float32, owned by the context): cx_grid_filter3d_bind"
        self._bind_pending(self.filter_result, self.lib.cx_grid_filter3d_bind)

    def distance_grid(self, value, side="below", kind="float32", sampling=None, radius2=0.0, samples=None, out=None, download=False):
        """exact Euclidean distance transform of the samples thresholded at `value` (cx_grid_distance3d) -> (n_sites, the result).
        side: a name of DIST_SIDES; kind: a name of DIST_KINDS ("squared": float64 squared distances, "float32": distances, "mask":
        uint8, 1 where the squared distance is <= radius2); sampling: None or the three steps of the lattice.
        samples: as in filter_grid (None = the bound grid, a 3-D numpy array, (device pointer, dtype, shape), (numpy array, dtype, shape)).
        out: None = the result stays in the context (distance_result, bind_distance); or a device pointer to room for the result.
        The result: a numpy array of the kind's type with download=True, else its device pointer."""
        keep = []
        ptr, code, on_device, shape = locate_samples(samples, keep)
        steps = None if sampling is None else np.ascontiguousarray(sampling, dtype=np.float64).reshape(3)
        kind_code = DIST_KINDS[kind]
        if download:
            n = self.shape if samples is None else shape
            if n is None:
                raise CxError(CX_ERR_STATE, "distance_grid: no samples given and no grid bound")
            host_out = np.empty(n, dtype=DIST_KIND_DTYPES.get(kind_code, np.uint8))
        n_sites = ctypes.c_int64()
        self._check(self.lib.cx_grid_distance3d(self.handle, ptr, code, on_device, shape[0], shape[1], shape[2], float(value),
                                                None if steps is None else steps.ctypes.data, DIST_SIDES[side], kind_code, float(radius2),
                                                ctypes.c_void_p(int(out)) if out else None, host_out.ctypes.data if download else None,
                                                ctypes.addressof(n_sites)))
        if download:
            return int(n_sites.value), host_out
        return int(n_sites.value), (int(out) if out else self.distance_result()[1])

    def distance_result(self):
        "(shape, device pointer, kind name, n_sites) of the result the last distance_grid left in the context (cx_grid_distance3d_result)"
        p, m, kind, n_sites = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), ctypes.c_int32(), ctypes.c_int64()
        self._check(self.lib.cx_grid_distance3d_result(self.handle, ctypes.byref(p), m.ctypes.data, ctypes.byref(kind), ctypes.byref(n_sites)))
        names = {v: k for k, v in DIST_KINDS.items()}
        return tuple(int(x) for x in m), int(p.value or 0), names[int(kind.value)], int(n_sites.value)

    def bind_distance(self):
        """the float32 or mask result the last distance_grid left in the context becomes the bound grid (float32 / uint8, owned by the
        context): cx_grid_distance3d_bind"""
        self._bind_pending(self.distance_result, self.lib.cx_grid_distance3d_bind)

    def label_grid(self, value, side="high", connectivity=1, samples=None, out=None, download=False):
        """connected components of the samples thresholded at `value` (cx_grid_label3d) -> (K, the labels).
        side: a name of LABEL_SIDES ("high": the samples with f >= value and the NaNs are labelled, "low": those with f < value);
        connectivity: 1, 2 or 3 (6, 18 or 26 neighbours).
        samples: as in filter_grid (None = the bound grid, a 3-D numpy array, (device pointer, dtype, shape), (numpy array, dtype, shape)).
        out: None = the labels stay in the context (label_result, label_measures, label_select); or a device pointer to room for them.
        The labels: an int32 numpy array with download=True, else their device pointer."""
        keep = []
        ptr, code, on_device, shape = locate_samples(samples, keep)
        if download:
            n = self.shape if samples is None else shape
            if n is None:
                raise CxError(CX_ERR_STATE, "label_grid: no samples given and no grid bound")
            host_out = np.empty(n, dtype=np.int32)
        k = ctypes.c_int64()
        self._check(self.lib.cx_grid_label3d(self.handle, ptr, code, on_device, shape[0], shape[1], shape[2], float(value),
                                             LABEL_SIDES[side], int(connectivity), ctypes.c_void_p(int(out)) if out else None,
                                             host_out.ctypes.data if download else None, ctypes.addressof(k)))
        if download:
            return int(k.value), host_out
        return int(k.value), (int(out) if out else self.label_result()[1])

    def label_result(self):
        "(shape, device pointer, side name, connectivity, K) of the labels the last label_grid left in the context (cx_grid_label3d_result)"
        p, m, side, conn, k = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        self._check(self.lib.cx_grid_label3d_result(self.handle, ctypes.byref(p), m.ctypes.data, ctypes.byref(side), ctypes.byref(conn), ctypes.byref(k)))
        names = {v: n for n, v in LABEL_SIDES.items()}
        return tuple(int(x) for x in m), int(p.value or 0), names[int(side.value)], int(conn.value), int(k.value)

    def label_measures(self):
        "one record (LABEL_COMPONENT_DTYPE) per component of the labels in the context, record c - 1 for label c (cx_grid_label3d_measures)"
        k = self.label_result()[4]
        out = np.zeros(k, dtype=LABEL_COMPONENT_DTYPE)
        self._check(self.lib.cx_grid_label3d_measures(self.handle, out.ctypes.data if k else None, k))
        return out

    def label_select(self, keep, out=None, download=False):
        """uint8 mask, 1 where keep[label] is set (cx_grid_label3d_select) -> (number of ones, the mask).  keep: K + 1 flags indexed by
        label, keep[0] for the samples without one.  out: None = the mask stays in the context (label_mask_result, bind_label_mask); or
        a device pointer to room for it.  The mask: a numpy array with download=True, else its device pointer."""
        flags = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8).reshape(-1)
        if download:
            host_out = np.empty(self.label_result()[0], dtype=np.uint8)
        n = ctypes.c_int64()
        self._check(self.lib.cx_grid_label3d_select(self.handle, flags.ctypes.data, len(flags), ctypes.c_void_p(int(out)) if out else None,
                                                    host_out.ctypes.data if download else None, ctypes.addressof(n)))
        if download:
            return int(n.value), host_out
        return int(n.value), (int(out) if out else self.label_mask_result()[1])

    def label_mask_result(self):
        "(shape, device pointer, number of ones) of the mask the last label_select left in the context (cx_grid_label3d_select_result)"
        p, m, n = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), ctypes.c_int64()
        self._check(self.lib.cx_grid_label3d_select_result(self.handle, ctypes.byref(p), m.ctypes.data, ctypes.byref(n)))
        return tuple(int(x) for x in m), int(p.value or 0), int(n.value)

    def bind_label_mask(self):
        "the mask the last label_select left in the context becomes the bound grid (uint8, owned by the context): cx_grid_label3d_bind"
        self._bind_pending(self.label_mask_result, self.lib.cx_grid_label3d_bind)

    def resample_grid(self, matrix, offset, out_shape, order=1, mode="nearest", cval=0.0, samples=None, out=None, download=False):
        """the samples read through the affine index map c = offset + matrix @ i (cx_grid_resample3d) -> (n_outside, the result).
        matrix: 3 x 3, output index to input index (scipy.ndimage.affine_transform's convention); offset: 3; out_shape: 3.
        order 0: the nearest sample in the input's own type; order 1: trilinear, float32.  mode: a name of FILTER_MODES.
        samples: as in filter_grid (None = the bound grid, a 3-D numpy array, (device pointer, dtype, shape), (numpy array, dtype, shape)).
        out: None = the result stays in the context (resample_result, bind_resampled); or a device pointer to room for the result.
        The result: a numpy array with download=True (bfloat16 samples at order 0 come back as their uint16 bit patterns), else its
        device pointer.  n_outside: the output samples whose source coordinate lies off the array on some axis."""
        keep = []
        ptr, code, on_device, shape = locate_samples(samples, keep)
        mat = np.ascontiguousarray(matrix, dtype=np.float64).reshape(3, 3)
        off = np.ascontiguousarray(offset, dtype=np.float64).reshape(3)
        m = np.ascontiguousarray(out_shape, dtype=np.int64).reshape(3)
        if download:
            if samples is None:
                if self.shape is None:
                    raise CxError(CX_ERR_STATE, "resample_grid: no samples given and no grid bound")
                code = DTYPE_CODES[self.grid_info()["dtype"]]
            host_out = _download_array(m, code if int(order) == 0 else DTYPE_CODES["float32"])
        n_outside = ctypes.c_int64()
        self._check(self.lib.cx_grid_resample3d(self.handle, ptr, code, on_device, shape[0], shape[1], shape[2], mat.ctypes.data, off.ctypes.data,
                                                m.ctypes.data, int(order), FILTER_MODES[mode], float(cval), ctypes.c_void_p(int(out)) if out else None,
                                                host_out.ctypes.data if download else None, ctypes.addressof(n_outside)))
        if download:
            return int(n_outside.value), host_out
        return int(n_outside.value), (int(out) if out else self.resample_result()[1])

    def resample_result(self):
        "(shape, device pointer, dtype name, n_outside) of the result the last resample_grid left in the context (cx_grid_resample3d_result)"
        p, m, code, n_outside = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), ctypes.c_int32(), ctypes.c_int64()
        self._check(self.lib.cx_grid_resample3d_result(self.handle, ctypes.byref(p), m.ctypes.data, ctypes.byref(code), ctypes.byref(n_outside)))
        return tuple(int(x) for x in m), int(p.value or 0), DTYPE_NAMES[int(code.value)], int(n_outside.value)

    def bind_resampled(self):
        """the result the last resample_grid left in the context becomes the bound grid (float32 for order 1, the input's type for order 0,
        owned by the context): cx_grid_resample3d_bind"""
        self._bind_pending(self.resample_result, self.lib.cx_grid_resample3d_bind)

    def rank_grid(self, size, rank, footprint=None, origin=None, mode="nearest", cval=0, samples=None, out=None, download=False):
        """the element at position `rank` of the sorted window around every sample (cx_grid_rank3d) -> (shape, the result).
        size: the three sides of the footprint's box (or one for all), 1..7; footprint: None = the whole box, or an array of that shape, non-zero = the
        offset belongs to it; rank: 0 .. W - 1, W the number of offsets; origin: None = size // 2 per axis (scipy's centre), or three
        values 0 .. size - 1.  mode: a name of FILTER_MODES; cval: a value of the sample type.
        samples: as in filter_grid (None = the bound grid, a 3-D numpy array, (device pointer, dtype, shape), (numpy array, dtype, shape)).
        out: None = the result stays in the context (rank_result, bind_ranked); or a device pointer to room for the result.
        The result has the samples' type: a numpy array with download=True (bfloat16 samples come back as their uint16 bit patterns),
        else its device pointer."""
        keep = []
        ptr, code, on_device, shape = locate_samples(samples, keep)
        box = np.ascontiguousarray(np.broadcast_to(np.asarray(size, dtype=np.int32), (3,)))
        og = box // 2 if origin is None else np.ascontiguousarray(origin, dtype=np.int32).reshape(3)
        fp = None
        if footprint is not None:
            fp = np.ascontiguousarray(np.asarray(footprint) != 0, dtype=np.uint8)
            assert fp.shape == tuple(int(s) for s in box), "footprint: an array of the shape `size`"
        if samples is None:
            if self.shape is None:
                raise CxError(CX_ERR_STATE, "rank_grid: no samples given and no grid bound")
            shape_out, code_out = tuple(self.shape), DTYPE_CODES[self.grid_info()["dtype"]]
        else:
            shape_out, code_out = shape, code
        if download:
            host_out = _download_array(shape_out, code_out)
        self._check(self.lib.cx_grid_rank3d(self.handle, ptr, code, on_device, shape[0], shape[1], shape[2], box.ctypes.data, og.ctypes.data,
                                            None if fp is None else fp.ctypes.data, int(rank), FILTER_MODES[mode], float(cval),
                                            ctypes.c_void_p(int(out)) if out else None, host_out.ctypes.data if download else None))
        if download:
            return shape_out, host_out
        return shape_out, (int(out) if out else self.rank_result()[1])

    def rank_result(self):
        "(shape, device pointer, dtype name) of the result the last rank_grid left in the context (cx_grid_rank3d_result)"
        p, m, code = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), ctypes.c_int32()
        self._check(self.lib.cx_grid_rank3d_result(self.handle, ctypes.byref(p), m.ctypes.data, ctypes.byref(code)))
        return tuple(int(x) for x in m), int(p.value or 0), DTYPE_NAMES[int(code.value)]

    def bind_ranked(self):
        "the result the last rank_grid left in the context becomes the bound grid (the samples' own type, owned by the context): cx_grid_rank3d_bind"
        self._bind_pending(self.rank_result, self.lib.cx_grid_rank3d_bind)

    def reconstruct_grid(self, marker="step", h=0.0, faces=RECON_ALL_FACES, method="dilation", connectivity=1, out_kind="values", samples=None,
                         out=None, download=False):
        """grey morphological reconstruction under the mask `samples` (cx_grid_reconstruct3d) -> (stats, the result).
        marker: a name of RECON_MARKERS other than "array" ("shift": mask -+ h, "step": the predecessor / successor, "rim": the mask on
        the faces `faces`), or a marker array given the way `samples` is; method: a name of RECON_METHODS; connectivity: 1, 2 or 3;
        out_kind: a name of RECON_OUTS ("values": the samples' type, "changed": uint8, 1 where the result differs from the mask).
        samples: as in filter_grid (None = the bound grid, a 3-D numpy array, (device pointer, dtype, shape), (numpy array, dtype, shape));
        a marker array has the same form (a device pointer when samples is None) and the mask's shape and type.
        out: None = the result stays in the context (reconstruct_result, bind_reconstructed); or a device pointer to room for the result.
        stats: a dict of RECON_STATS (n_changed and n_clamped exact; rounds and tile_visits informational).  The result: a numpy array
        with download=True (bfloat16 samples come back as their uint16 bit patterns), else its device pointer."""
        keep = []
        ptr, code, on_device, shape = locate_samples(samples, keep)
        if samples is None:
            if self.shape is None:
                raise CxError(CX_ERR_STATE, "reconstruct_grid: no samples given and no grid bound")
            shape_out, code_out = tuple(self.shape), DTYPE_CODES[self.grid_info()["dtype"]]
        else:
            shape_out, code_out = shape, code
        mptr = None
        if isinstance(marker, str):
            kind = RECON_MARKERS[marker]
            assert marker != "array", "marker: the array itself, or the name of another marker kind"
        elif marker is None:
            kind = RECON_MARKERS["array"]      # (refused by the library)
        else:
            kind = RECON_MARKERS["array"]
            mptr, mcode, m_on_device, mshape = locate_samples(marker, keep)
            assert mcode == code_out and tuple(mshape) == tuple(shape_out) and m_on_device == on_device, "marker: the mask's shape, type and residency"
        if download:
            host_out = _download_array(shape_out, code_out if RECON_OUTS[out_kind] == 0 else DTYPE_CODES["uint8"])
        st = np.zeros(4, dtype=np.int64)
        self._check(self.lib.cx_grid_reconstruct3d(self.handle, ptr, code, on_device, shape[0], shape[1], shape[2], mptr, kind, float(h), int(faces),
                                                   RECON_METHODS[method], int(connectivity), RECON_OUTS[out_kind],
                                                   ctypes.c_void_p(int(out)) if out else None, host_out.ctypes.data if download else None,
                                                   st.ctypes.data))
        stats = dict(zip(RECON_STATS, (int(x) for x in st)))
        if download:
            return stats, host_out
        return stats, (int(out) if out else self.reconstruct_result()[1])

    def reconstruct_result(self):
        "(shape, device pointer, dtype name, out kind name) of the result the last reconstruct_grid left in the context (cx_grid_reconstruct3d_result)"
        p, m, code, kind = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.cx_grid_reconstruct3d_result(self.handle, ctypes.byref(p), m.ctypes.data, ctypes.byref(code), ctypes.byref(kind)))
        names = {v: k for k, v in RECON_OUTS.items()}
        return tuple(int(x) for x in m), int(p.value or 0), DTYPE_NAMES[int(code.value)], names[int(kind.value)]

    def bind_reconstructed(self):
        """the result the last reconstruct_grid left in the context becomes the bound grid (the samples' own type, uint8 for "changed", owned
        by the context): cx_grid_reconstruct3d_bind"""
        self._bind_pending(self.reconstruct_result, self.lib.cx_grid_reconstruct3d_bind)

    def watershed_grid(self, markers, region=None, connectivity=1, direction="rising", samples=None, out=None, out_host=None):
        """marker-based watershed of the relief `samples` (cx_grid_watershed3d) -> (stats, the labels).
        samples: as in filter_grid (None = the bound grid, a 3-D numpy array, (device pointer, dtype, shape), (numpy array, dtype, shape)).
        markers: int32 of the relief's shape, a value above 0 a label: a numpy array beside host samples, a device pointer beside
        samples on the device (or the bound grid).  region: None = every sample, or uint8 given the way the markers are, non-zero =
        inside.  connectivity: 1, 2 or 3; direction: a name of WATERSHED_DIRECTIONS ("falling" floods from the maxima down).
        out: None = the labels stay in the context (watershed_result); or a device pointer to room for n int32.  out_host: None, True
        (a new int32 array) or a contiguous int32 array of the relief's shape, which receives a copy.
        stats: a dict of WATERSHED_STATS (the first four exact, the last three informational).  The labels: the host array with
        out_host, else their device pointer."""
        keep = []
        ptr, code, on_device, shape = locate_samples(samples, keep)
        if samples is None:
            if self.shape is None:
                raise CxError(CX_ERR_STATE, "watershed_grid: no samples given and no grid bound")
            shape = tuple(self.shape)

        def beside(a, dtype, name):
            "the pointer of an array that lives where the samples do"
            if a is None:
                return None
            if on_device:
                assert not isinstance(a, np.ndarray), "%s: a device pointer beside samples on the device" % name
                return ctypes.c_void_p(int(a))
            h = np.ascontiguousarray(a, dtype=dtype)
            assert h.shape == tuple(shape), "%s: the shape of the samples" % name
            keep.append(h)
            return ctypes.c_void_p(h.ctypes.data)
        mptr = beside(markers, np.int32, "markers")
        rptr = beside(region, np.uint8, "region")
        host_out = None
        if out_host is True:
            host_out = np.empty(shape, dtype=np.int32)
        elif out_host is not None:
            host_out = out_host
            assert isinstance(host_out, np.ndarray) and host_out.dtype == np.int32 and host_out.flags.c_contiguous and host_out.shape == tuple(shape), \
                "out_host: a contiguous int32 array of the samples' shape"
        st = np.zeros(len(WATERSHED_STATS), dtype=np.int64)
        self._check(self.lib.cx_grid_watershed3d(self.handle, ptr, code, on_device, shape[0] if samples is not None else 0,
                                                 shape[1] if samples is not None else 0, shape[2] if samples is not None else 0, mptr, rptr,
                                                 int(connectivity), WATERSHED_DIRECTIONS[direction], ctypes.c_void_p(int(out)) if out else None,
                                                 None if host_out is None else host_out.ctypes.data, st.ctypes.data))
        stats = dict(zip(WATERSHED_STATS, (int(x) for x in st)))
        if host_out is not None:
            return stats, host_out
        return stats, (int(out) if out else self.watershed_result()[1])

    def watershed_result(self):
        "(shape, device pointer) of the labels the last watershed_grid left in the context (cx_grid_watershed3d_result)"
        p, m = ctypes.c_void_p(), np.zeros(3, dtype=np.int64)
        self._check(self.lib.cx_grid_watershed3d_result(self.handle, ctypes.byref(p), m.ctypes.data))
        return tuple(int(x) for x in m), int(p.value or 0)

    @staticmethod
    def _locate_labels(labels, keep):
        """the labels of a regions call -> (pointer, on_device, shape): a 3-D numpy array (made int32 and contiguous, appended to `keep`)
        or (device pointer, shape) of contiguous int32 labels on the device"""
        if isinstance(labels, tuple):
            ptr, shape = labels
            shape = tuple(int(n) for n in shape)
            assert len(shape) == 3, "3-D label array expected"
            return ctypes.c_void_p(int(ptr)), 1, shape
        host = np.ascontiguousarray(labels, dtype=np.int32)
        assert host.ndim == 3, "3-D label array expected"
        keep.append(host)
        return ctypes.c_void_p(host.ctypes.data), 0, tuple(int(n) for n in host.shape)

    def regions_grid(self, labels, values=None, count_only=False):
        """one record (REGION_DTYPE) per label 1 .. K of an int32 label volume, K its largest label (cx_grid_regions3d); record c - 1
        belongs to label c.  labels: a 3-D numpy array or (device pointer, shape).  values: None, or a second array of the labels' shape
        given as `samples` is elsewhere (a numpy array of a type of DTYPE_CODES, (device pointer, dtype, shape), (numpy array, dtype,
        shape)): the records then carry its extremes, their places and its sums per label.  count_only: -> (K, number of negative
        labels) and no records."""
        keep = []
        lptr, on_device, shape = self._locate_labels(labels, keep)
        vptr, vcode, v_on_device = None, 0, 0
        if values is not None:
            vptr, vcode, v_on_device, vshape = locate_samples(values, keep)
            assert vshape == shape, "values: the shape of the labels"
        k, neg = ctypes.c_int64(), ctypes.c_int64()
        head = (self.handle, lptr, on_device, shape[0], shape[1], shape[2], vptr, vcode, v_on_device)
        self._check(self.lib.cx_grid_regions3d(*head, None, 0, ctypes.addressof(k), ctypes.addressof(neg)))
        if count_only:
            return int(k.value), int(neg.value)
        out = np.zeros(int(k.value), dtype=REGION_DTYPE)
        if len(out):
            self._check(self.lib.cx_grid_regions3d(*head, out.ctypes.data, len(out), None, None))
        return out

    def regions_select(self, labels, keep, box=None, pad=0, out=None, download=False):
        """uint8 mask of the labels whose keep flag is set, cropped to a box grown by `pad` (cx_grid_regions3d_select) ->
        (number of ones, shape, origin, the mask).  keep: flags indexed by label, keep[0] for the background; labels beyond it are not
        kept.  box: None = the whole array, or (lo, hi), index triples, both ends included; pad: 0 .. 8, the rim of zeros where it
        leaves the array.  origin = lo - pad, the place of the mask's first sample in the labels' indices (may be negative).
        out: None = the mask stays in the context (regions_mask_result, bind_region_mask); or a device pointer to room for it.
        The mask: a numpy array with download=True, else its device pointer."""
        held = []
        lptr, on_device, shape = self._locate_labels(labels, held)
        flags = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8).reshape(-1)
        lo = hi = None
        if box is not None:
            lo = np.ascontiguousarray(box[0], dtype=np.int64).reshape(3)
            hi = np.ascontiguousarray(box[1], dtype=np.int64).reshape(3)
        host_out = None
        if download:
            ext = [(int(hi[a] - lo[a]) + 1 if box is not None else shape[a]) + 2 * int(pad) for a in range(3)]
            host_out = np.empty([max(0, e) for e in ext], dtype=np.uint8)
        m, org, n = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), ctypes.c_int64()
        self._check(self.lib.cx_grid_regions3d_select(self.handle, lptr, on_device, shape[0], shape[1], shape[2], flags.ctypes.data if len(flags) else None,
                                                      len(flags), None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data, int(pad),
                                                      ctypes.c_void_p(int(out)) if out else None, None if host_out is None else host_out.ctypes.data,
                                                      m.ctypes.data, org.ctypes.data, ctypes.addressof(n)))
        shape_out, origin = tuple(int(x) for x in m), tuple(int(x) for x in org)
        if download:
            assert host_out.shape == shape_out
            return int(n.value), shape_out, origin, host_out
        return int(n.value), shape_out, origin, (int(out) if out else self.regions_mask_result()[1])

    def regions_mask_result(self):
        "(shape, device pointer, origin, number of ones) of the mask the last regions_select left in the context (cx_grid_regions3d_select_result)"
        p, m, org, n = ctypes.c_void_p(), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), ctypes.c_int64()
        self._check(self.lib.cx_grid_regions3d_select_result(self.handle, ctypes.byref(p), m.ctypes.data, org.ctypes.data, ctypes.byref(n)))
        return tuple(int(x) for x in m), int(p.value or 0), tuple(int(x) for x in org), int(n.value)

    def bind_region_mask(self):
        """the mask the last regions_select left in the context becomes the bound grid (uint8, owned by the context): cx_grid_regions3d_bind.
        The origin stays what set_origin made it, as across uploads: set_origin(*origin) of the mask makes the march of the crop the
        march of the whole mask."""
        self._bind_pending(self.regions_mask_result, self.lib.cx_grid_regions3d_bind)

    def regions_map(self, labels, table, out=None, download=False):
        """out = table[label], 0 for labels beyond the table (cx_grid_regions3d_map) -> the mapped labels: a numpy array with
        download=True, else the device pointer `out`, which may be the labels' own pointer (in place).  table: int32 indexed by label."""
        held = []
        lptr, on_device, shape = self._locate_labels(labels, held)
        tab = np.ascontiguousarray(table, dtype=np.int32).reshape(-1)
        assert out or download, "regions_map: a device pointer to write to, or download=True"
        host_out = np.empty(shape, dtype=np.int32) if download else None
        self._check(self.lib.cx_grid_regions3d_map(self.handle, lptr, on_device, shape[0], shape[1], shape[2], tab.ctypes.data if len(tab) else None, len(tab),
                                                   ctypes.c_void_p(int(out)) if out else None, None if host_out is None else host_out.ctypes.data))
        return host_out if download else int(out)

    def regions_contacts(self, labels):
        """the pairs of labels that share a face (cx_grid_regions3d_contacts) -> records of REGION_CONTACT_DTYPE sorted by (a, b), a < b,
        0 (the background) included as a partner; faces[x]: the sample pairs adjacent along axis x that carry the two labels"""
        held = []
        lptr, on_device, shape = self._locate_labels(labels, held)
        n = ctypes.c_int64()
        head = (self.handle, lptr, on_device, shape[0], shape[1], shape[2])
        out = np.zeros(4096, dtype=REGION_CONTACT_DTYPE)      # most volumes have fewer pairs: one pass; else the count, then a second pass
        rc = self.lib.cx_grid_regions3d_contacts(*head, out.ctypes.data, len(out), ctypes.addressof(n))
        if rc == CX_ERR_INVALID and n.value > len(out):
            out = np.zeros(int(n.value), dtype=REGION_CONTACT_DTYPE)
            rc = self.lib.cx_grid_regions3d_contacts(*head, out.ctypes.data, len(out), ctypes.addressof(n))
        self._check(rc)
        return out[:int(n.value)].copy()

    def level0_points_f64(self, counts):
        "float64 coordinates of the Level-0 vertices as the reference interpolates them, in download_level0 order"
        pts = np.empty((int(counts["n_vertices"]), 3), dtype=np.float64)
        self._check(self.lib.cx_level0_points_f64(self.handle, pts.ctypes.data))
        return pts

    def postprocess3d_mesh(self, points, triangles, corner, flags=0, smooth=0.0):
        """Level 1 of an assembled Level-0 mesh (vertices in ascending global edge-id order, float64 grid coordinates of
        the whole volume, triangles as indices) -> the same dict as postprocess3d; fetch with download_level1"""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        tris = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
        c3 = np.ascontiguousarray(corner, dtype=np.int64).reshape(3)
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_postprocess3d_mesh(self.handle, pts.ctypes.data, len(pts), tris.ctypes.data, len(tris), c3.ctypes.data,
                                                   int(flags), float(smooth or 0.0), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_after_weld=int(out[2]),
                    n_after_tiny=int(out[3]), n_components=int(out[4]))

    def download_level1(self, counts):
        pts = np.empty((int(counts["n_vertices"]), 3), dtype=np.float64)
        tris = np.empty((int(counts["n_triangles"]), 3), dtype=np.int32)
        self._check(self.lib.cx_level1_download(self.handle, pts.ctypes.data, tris.ctypes.data))
        return pts, tris

    def level1_device_ptrs(self):
        "(points pointer, triangles pointer, n_vertices, n_triangles) of the Level-1 mesh ON THE DEVICE (no copy; valid until the next post-pass)"
        pp, tp, nv, nt = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.cx_level1_device_ptrs(self.handle, ctypes.byref(pp), ctypes.byref(tp), ctypes.byref(nv), ctypes.byref(nt)))
        return pp.value or 0, tp.value or 0, nv.value, nt.value

    def level1_torch(self, copy=True):
        """the Level-1 mesh as torch tensors on the context's device: points (V,3) float64, triangles (T,3) int32 (device order).
        copy=True: tensors that own their memory (one device-to-device copy); copy=False: views of the context's buffers,
        valid only until the next post-pass / extraction on this context."""
        import torch
        pp, tp, nv, nt = self.level1_device_ptrs()
        dev = torch.device("cuda", self.device)

        class _View(object):
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        pts = torch.as_tensor(_View(pp, (nv, 3), "<f8"), device=dev) if nv else torch.zeros((0, 3), dtype=torch.float64, device=dev)
        tris = torch.as_tensor(_View(tp, (nt, 3), "<i4"), device=dev) if nt else torch.zeros((0, 3), dtype=torch.int32, device=dev)
        if copy:
            pts, tris = pts.clone(), tris.clone()
        else:
            pts._cx_keep = tris._cx_keep = self
        return pts, tris

    def download_level1_keys(self, counts):
        "edge ids (local to the marched array) of the vertices of download_level1, in its order"
        keys = np.empty(int(counts["n_vertices"]), dtype=np.uint32)
        self._check(self.lib.cx_level1_download_keys(self.handle, keys.ctypes.data))
        return keys

    def shard_begin(self, own_lo, own_hi, flags=0):
        """sharded Level 1, local part (cx_postprocess3d_shard_begin + _candidates) -> dict(counts, n_own_lower, n_upper_copies,
        cand_label / cand_x / cand_vertex_key / cand_nx / cand_negative / cand_has (C,)); the boundary lists stay on the device
        (shard_boundary)"""
        out = np.zeros(8, dtype=np.int64)
        n1, n4, nc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.lib.cx_postprocess3d_shard_begin(self.handle, int(flags), int(own_lo), int(own_hi), out.ctypes.data,
                                                          ctypes.addressof(n1), ctypes.addressof(n4), ctypes.addressof(nc)))
        C = int(nc.value)
        L = dict(cand_label=np.zeros(C, np.uint32), cand_x=np.zeros(C, np.float64), cand_vertex_key=np.zeros(C, np.uint32),
                 cand_nx=np.zeros(C, np.float64), cand_negative=np.zeros(C, np.uint8), cand_has=np.zeros(C, np.uint8))
        if C:
            self._check(self.lib.cx_postprocess3d_shard_candidates(self.handle, *[L[k].ctypes.data for k in (
                "cand_label", "cand_x", "cand_vertex_key", "cand_nx", "cand_negative", "cand_has")]))
        L.update(n_own_lower=int(n1.value), n_upper_copies=int(n4.value), counts=dict(n_after_weld=int(out[2]), n_after_tiny=int(out[3])))
        return L

    def shard_boundary(self, which, n, torch_device=None):
        """one boundary list of shard_begin (which = 1: own triangles next to the lower neighbour, 4: copies of the upper
        neighbour's first layer) -> (hash int64 (n,), label int32 (n,)): torch tensors on `torch_device` (the lists need not
        leave the GPU), numpy arrays without one.  The hashes are 64-bit patterns; as int64 they sort the same way on every rank."""
        n = int(n)
        if torch_device is not None:
            import torch
            h = torch.empty(n, dtype=torch.int64, device=torch_device)
            lab = torch.empty(n, dtype=torch.int32, device=torch_device)
            hp, lp = h.data_ptr(), lab.data_ptr()
        else:
            h = np.empty(n, dtype=np.int64)
            lab = np.empty(n, dtype=np.int32)
            hp, lp = h.ctypes.data, lab.ctypes.data
        if n:
            self._check(self.lib.cx_postprocess3d_shard_boundary(self.handle, int(which), ctypes.c_void_p(hp), ctypes.c_void_p(lp)))
        return h, lab

    def shard_finish(self, labels, flips):
        "the agreed flips for the components that reach a neighbour -> counts dict for download_level1 / download_level1_keys"
        lab = np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)
        fl = np.ascontiguousarray(flips, dtype=np.uint8).reshape(-1)
        assert len(lab) == len(fl)
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_postprocess3d_shard_finish(self.handle, lab.ctypes.data if len(lab) else None, fl.ctypes.data if len(fl) else None,
                                                           len(lab), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_components=int(out[4]))

    def write_level1(self, path, fmt="ply", mins=None, delta=None):
        """the Level-1 mesh of the last post-pass as a binary file written straight from the device buffers (no numpy arrays):
        fmt "ply" (float64 positions, int32 faces), "gltf_bin" (float32 positions + uint32 indices), "ply_normals" (double nx ny nz
        after x y z) or "gltf_bin_normals" (float32 positions, float32 normals, uint32 indices); mins / delta: world
        coordinates = grid * delta + mins.  -> dict(n_vertices, n_triangles, bytes, min, max)"""
        md = None
        if mins is not None or delta is not None:
            md = np.ascontiguousarray(np.concatenate([np.asarray(mins if mins is not None else [0, 0, 0], dtype=np.float64).reshape(3),
                                                      np.asarray(delta if delta is not None else [1, 1, 1], dtype=np.float64).reshape(3)]))
        info = np.zeros(9, dtype=np.float64)
        self._check_attr(self.lib.cx_level1_write(self.handle, {"ply": 0, "gltf_bin": 1, "ply_normals": 2, "gltf_bin_normals": 3}[fmt], os.fsencode(path),
                                             None if md is None else md.ctypes.data, info.ctypes.data))
        return dict(n_vertices=int(info[0]), n_triangles=int(info[1]), bytes=int(info[2]), min=info[3:6].copy(), max=info[6:9].copy())

    # ---- vertex attributes (cx_attr.hip): normals from the field's gradient, a second grid sampled at the vertices ----------
    def _check_attr(self, rc):
        "CX_ERR_UNSUPPORTED of the attribute calls is a NotImplementedError with the library's plain message"
        if rc == CX_ERR_UNSUPPORTED:
            raise NotImplementedError(self.lib.cx_last_error(self.handle).decode("utf-8", "replace"))
        self._check(rc)

    @staticmethod
    def _delta3(delta):
        return None if delta is None else np.ascontiguousarray(np.asarray(delta, dtype=np.float64).reshape(3))

    def _device_view(self, ptr, shape, typestr, torch_dtype):
        "a torch tensor that owns a copy of `shape` elements at device address `ptr` (an empty one for ptr == 0)"
        import torch
        dev = torch.device("cuda", self.device)
        if not ptr or not shape[0]:
            return torch.zeros(shape, dtype=torch_dtype, device=dev)

        class _View(object):
            def __init__(self, ptr, shape, typestr):
                self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2, "strides": None}
        self.synchronize()
        return torch.as_tensor(_View(ptr, shape, typestr), device=dev).clone()

    def level0_normals(self, counts, delta=None, device=False):
        """(V,4) float32 {nx, ny, nz, |g|} per vertex record of the current extraction, in the order of download_level0
        (delta: world spacing per axis; device=True: a torch tensor on the GPU)"""
        nv = int(counts["n_vertices"])
        d3 = self._delta3(delta)
        dp = None if d3 is None else d3.ctypes.data
        if device:
            import torch
            p = ctypes.c_void_p()
            self._check_attr(self.lib.cx_level0_normals(self.handle, dp, ctypes.byref(p)))
            return self._device_view(p.value or 0, (nv, 4), "<f4", torch.float32)
        out = np.zeros((nv, 4), dtype=np.float32)
        self._check_attr(self.lib.cx_level0_normals_download(self.handle, dp, out.ctypes.data))
        return out

    def level1_normals(self, counts, delta=None, device=False):
        """(V,3) float64 unit normals of the Level-1 vertices in the order of download_level1, agreeing with the winding of
        their triangles (delta: world spacing per axis; device=True: a torch tensor on the GPU)"""
        nv = int(counts["n_vertices"])
        d3 = self._delta3(delta)
        dp = None if d3 is None else d3.ctypes.data
        if device:
            import torch
            p = ctypes.c_void_p()
            self._check_attr(self.lib.cx_level1_normals(self.handle, dp, ctypes.byref(p)))
            return self._device_view(p.value or 0, (nv, 3), "<f8", torch.float64)
        out = np.zeros((nv, 3), dtype=np.float64)
        self._check_attr(self.lib.cx_level1_normals_download(self.handle, dp, out.ctypes.data))
        return out

    def level0_curvature(self, counts, delta=None, device=False):
        """(V,4) float32 {mean, gauss, k1, k2} per vertex record of the current extraction, in the order of download_level0
        (delta: world spacing per axis; device=True: a torch tensor on the GPU)"""
        nv = int(counts["n_vertices"])
        d3 = self._delta3(delta)
        dp = None if d3 is None else d3.ctypes.data
        if device:
            import torch
            p = ctypes.c_void_p()
            self._check_attr(self.lib.cx_level0_curvature(self.handle, dp, ctypes.byref(p)))
            return self._device_view(p.value or 0, (nv, 4), "<f4", torch.float32)
        out = np.zeros((nv, 4), dtype=np.float32)
        self._check_attr(self.lib.cx_level0_curvature_download(self.handle, dp, out.ctypes.data))
        return out

    def level1_curvature(self, counts, delta=None, device=False):
        """(V,4) float64 {mean, gauss, k1, k2} of the Level-1 vertices in the order of download_level1, signed like
        level1_normals (delta: world spacing per axis; device=True: a torch tensor on the GPU)"""
        nv = int(counts["n_vertices"])
        d3 = self._delta3(delta)
        dp = None if d3 is None else d3.ctypes.data
        if device:
            import torch
            p = ctypes.c_void_p()
            self._check_attr(self.lib.cx_level1_curvature(self.handle, dp, ctypes.byref(p)))
            return self._device_view(p.value or 0, (nv, 4), "<f8", torch.float64)
        out = np.zeros((nv, 4), dtype=np.float64)
        self._check_attr(self.lib.cx_level1_curvature_download(self.handle, dp, out.ctypes.data))
        return out

    def _second_grid(self, field):
        "(pointer, CX_DTYPE code, on_device, keepalive) of a second grid of the bound grid's shape, in its own type when the kernels read it"
        if hasattr(field, "data_ptr"):     # a torch tensor
            assert tuple(int(n) for n in field.shape) == tuple(self.shape), (tuple(field.shape), self.shape)
            t = field if native_dtype(field.dtype) else field.float()
            t = t.contiguous()
            if t.is_cuda:
                return t.data_ptr(), dtype_code(t.dtype), 1, t
            field = t.numpy() if str(t.dtype) != "torch.bfloat16" else t.float().numpy()
        a = np.asarray(field)
        assert tuple(a.shape) == tuple(self.shape), (a.shape, self.shape)
        a = native_array(a) if native_dtype(a.dtype) else np.ascontiguousarray(a, dtype=np.float32)
        return a.ctypes.data, dtype_code(a.dtype), 0, a

    def level0_sample(self, counts, field, device=False):
        "(V,) float32: `field` (an array or device tensor of the bound grid's shape) at the Level-0 vertices, B(q) + t (B(q+d) - B(q))"
        nv = int(counts["n_vertices"])
        ptr, code, on_dev, keep = self._second_grid(field)
        p = ctypes.c_void_p()
        if device:
            import torch
            self._check_attr(self.lib.cx_level0_sample_grid(self.handle, ctypes.c_void_p(ptr), code, on_dev, ctypes.byref(p), None))
            return self._device_view(p.value or 0, (nv,), "<f4", torch.float32)
        out = np.zeros(nv, dtype=np.float32)
        self._check_attr(self.lib.cx_level0_sample_grid(self.handle, ctypes.c_void_p(ptr), code, on_dev, ctypes.byref(p), out.ctypes.data))
        del keep
        return out

    def level1_sample(self, counts, field, device=False):
        "(V,) float64: `field` at the Level-1 vertices, B(low) + ratio (B(high) - B(low)), in the order of download_level1"
        nv = int(counts["n_vertices"])
        ptr, code, on_dev, keep = self._second_grid(field)
        p = ctypes.c_void_p()
        if device:
            import torch
            self._check_attr(self.lib.cx_level1_sample_grid(self.handle, ctypes.c_void_p(ptr), code, on_dev, ctypes.byref(p), None))
            return self._device_view(p.value or 0, (nv,), "<f8", torch.float64)
        out = np.zeros(nv, dtype=np.float64)
        self._check_attr(self.lib.cx_level1_sample_grid(self.handle, ctypes.c_void_p(ptr), code, on_dev, ctypes.byref(p), out.ctypes.data))
        del keep
        return out

    # ---- components of the Level-1 mesh (cx_comp.hip): labels, per-component measures, filtering ------------------------------
    @staticmethod
    def _mins_delta(mins, delta):
        if mins is None and delta is None:
            return None
        return np.ascontiguousarray(np.concatenate([np.asarray(mins if mins is not None else [0, 0, 0], dtype=np.float64).reshape(3),
                                                    np.asarray(delta if delta is not None else [1, 1, 1], dtype=np.float64).reshape(3)]))

    def level1_components(self, mins=None, delta=None, info=False):
        """the components of the Level-1 mesh as a numpy structured array (COMPONENT_DTYPE: triangles, vertices, area, volume,
        centroid, bbox_lo, bbox_hi, flipped, closed, first_triangle), in world coordinates grid * delta + mins when either is given.
        info=True: (table, origin (3,), q): the point the volumes are taken about and the exponent of the sums' grid 2^-q"""
        md = self._mins_delta(mins, delta)
        mp = None if md is None else md.ctypes.data
        nc, oq = ctypes.c_int64(0), np.zeros(4, dtype=np.float64)
        self._check_attr(self.lib.cx_level1_components(self.handle, mp, ctypes.byref(nc), None, oq.ctypes.data))
        table = np.zeros(int(nc.value), dtype=COMPONENT_DTYPE)
        if len(table):
            self._check_attr(self.lib.cx_level1_components_download(self.handle, mp, table.ctypes.data))
        return (table, oq[:3].copy(), int(oq[3])) if info else table

    def level1_component_labels(self, device=False):
        """(triangle labels int32 (T,), vertex labels int32 (V,)) of the Level-1 mesh in device order (a vertex: the smallest id
        among its triangles' components, -1 when unused); device=True: torch tensors on the GPU"""
        _pp, _tp, nv, nt = self.level1_device_ptrs()
        if device:
            import torch
            tp, vp = ctypes.c_void_p(), ctypes.c_void_p()
            self._check_attr(self.lib.cx_level1_component_labels(self.handle, ctypes.byref(tp), ctypes.byref(vp)))
            return (self._device_view(tp.value or 0, (nt,), "<i4", torch.int32), self._device_view(vp.value or 0, (nv,), "<i4", torch.int32))
        tl, vl = np.zeros(nt, dtype=np.int32), np.zeros(nv, dtype=np.int32)
        self._check_attr(self.lib.cx_level1_component_labels_download(self.handle, tl.ctypes.data, vl.ctypes.data))
        return tl, vl

    def level1_keep_components(self, mask):
        """drop the components whose entry of `mask` (one per component) is false; every reader of the Level-1 mesh serves the
        filtered mesh afterwards -> dict(n_vertices, n_triangles, n_components)"""
        keep = np.ascontiguousarray(np.asarray(mask).astype(bool), dtype=np.uint8).reshape(-1)
        nc = ctypes.c_int64(0)
        self._check_attr(self.lib.cx_level1_components(self.handle, None, ctypes.byref(nc), None, None))
        if len(keep) != int(nc.value):
            raise ValueError("the mask has %d entries, the mesh has %d components" % (len(keep), int(nc.value)))
        out = np.zeros(8, dtype=np.int64)
        self._check_attr(self.lib.cx_level1_keep_components(self.handle, keep.ctypes.data if len(keep) else None, out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_components=int(out[4]))

    # ---- topology of the Level-1 mesh (cx_topo.hip): Euler number, genus, boundary loops ----------------------------------------
    def level1_topology(self, device=False):
        """the topology of the Level-1 mesh's components as a numpy structured array (TOPOLOGY_DTYPE: triangles, vertices, edges,
        boundary_edges, nonmanifold_edges, euler, boundary_loops, genus, nonsimple_loops), row c = component c.
        device=True: the records as a torch int32 tensor (nc, 16) on the GPU (64 bytes per row, the layout of cx_topology)"""
        nc, p = ctypes.c_int64(0), ctypes.c_void_p()
        self._check_attr(self.lib.cx_level1_topology(self.handle, ctypes.byref(nc), ctypes.byref(p)))
        if device:
            import torch
            return self._device_view(p.value or 0, (int(nc.value), 16), "<i4", torch.int32)
        table = np.zeros(int(nc.value), dtype=TOPOLOGY_DTYPE)
        if len(table):
            self._check_attr(self.lib.cx_level1_topology_download(self.handle, table.ctypes.data))
        return table

    def level1_boundary_loops(self, device=False):
        """(loops, vertices): the boundary loops of the Level-1 mesh as a numpy structured array (LOOP_DTYPE: component, simple,
        first, count) and the int32 vertex indices (device order of the points) of all loops, loop l in
        vertices[first : first + count]: in cyclic order for a simple loop, the tails of its edges for a non-simple one.
        device=True: torch int32 tensors on the GPU, the loops as (L, 4) rows in the layout of cx_loop"""
        nl, nb, lp, vp = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_void_p(), ctypes.c_void_p()
        self._check_attr(self.lib.cx_level1_boundary_loops(self.handle, ctypes.byref(nl), ctypes.byref(nb), ctypes.byref(lp), ctypes.byref(vp)))
        if device:
            import torch
            return (self._device_view(lp.value or 0, (int(nl.value), 4), "<i4", torch.int32),
                    self._device_view(vp.value or 0, (int(nb.value),), "<i4", torch.int32))
        loops, verts = np.zeros(int(nl.value), dtype=LOOP_DTYPE), np.zeros(int(nb.value), dtype=np.int32)
        if len(loops) or len(verts):
            self._check_attr(self.lib.cx_level1_boundary_loops_download(self.handle, loops.ctypes.data if len(loops) else None,
                                                                         verts.ctypes.data if len(verts) else None))
        return loops, verts

    # ---- simplification of the Level-1 mesh by vertex clustering (cx_simplify.hip) ----------------------------------------------
    def level1_simplify(self, cell, flags=0):
        """cx_level1_simplify with `cell` (a scalar or three, grid units) -> dict(n_vertices, n_triangles, n_components, n_clusters,
        cell, clamped, n_distinct, q); with CX_SIMPLIFY_COUNT_ONLY only n_clusters and n_distinct (triangles with three distinct
        indices after the remap) are filled and the mesh stays as it is"""
        c3 = np.ascontiguousarray(np.broadcast_to(np.asarray(cell, dtype=np.float64), (3,)))
        out, q = np.zeros(8, dtype=np.int64), ctypes.c_double(0.0)
        self._check_attr(self.lib.cx_level1_simplify(self.handle, c3.ctypes.data, int(flags), out.ctypes.data, ctypes.byref(q)))
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_components=int(out[4]), n_clusters=int(out[6]),
                    cell=tuple(float(c) for c in c3), clamped=int(out[5]), n_distinct=int(out[7]), q=int(q.value))

    def level1_simplify_map(self, n_old, device=False):
        "(n_old,) int32: the new index of every vertex of the mesh before the last simplification, -1 where it went away"
        n_old = int(n_old)
        if device:
            import torch
            p = ctypes.c_void_p()
            self._check_attr(self.lib.cx_level1_simplify_map(self.handle, ctypes.byref(p)))
            return self._device_view(p.value or 0, (n_old,), "<i4", torch.int32)
        out = np.zeros(n_old, dtype=np.int32)
        self._check_attr(self.lib.cx_level1_simplify_map_download(self.handle, out.ctypes.data if n_old else None))
        return out

    # ---- clipping of the Level-1 mesh by a plane or a per-vertex scalar (cx_clip.hip) --------------------------------------------
    @staticmethod
    def _clip_counts(out):
        return dict(n_vertices=int(out[0]), n_triangles=int(out[1]), n_components=int(out[4]), n_cut_vertices=int(out[2]),
                    n_cut_triangles=int(out[3]), n_nonfinite=int(out[5]), n_on_cut=int(out[6]), n_raw_triangles=int(out[7]))

    def level1_clip_plane(self, normal, offset, flags=0):
        """cx_level1_clip_plane: keep n.p >= offset (grid coordinates; n.p <= offset with CX_CLIP_KEEP_BELOW) -> dict(CLIP_KEYS
        and n_raw_triangles, the triangles handed to the tail)"""
        p4 = np.ascontiguousarray(np.concatenate([np.asarray(normal, dtype=np.float64).reshape(3), [float(offset)]]))
        out = np.zeros(8, dtype=np.int64)
        self._check_attr(self.lib.cx_level1_clip_plane(self.handle, p4.ctypes.data, int(flags), out.ctypes.data))
        return self._clip_counts(out)

    def level1_clip_scalars(self, scalars, threshold=0.0, flags=0):
        """cx_level1_clip_scalars: `scalars` one value per Level-1 vertex, a numpy array (converted to float64) or a torch tensor
        on the context's device; keeps scalars >= threshold -> the dict of level1_clip_plane"""
        nv = self.level1_device_ptrs()[2]
        out = np.zeros(8, dtype=np.int64)
        if hasattr(scalars, "data_ptr"):
            import torch
            t = scalars.reshape(-1).to(torch.float64).contiguous()
            if int(t.numel()) != nv:
                raise ValueError("%d scalars for %d vertices" % (int(t.numel()), nv))
            if t.is_cuda:
                if t.device.index not in (None, self.device):
                    t = t.to(torch.device("cuda", self.device))
                torch.cuda.synchronize(t.device)
                self._check_attr(self.lib.cx_level1_clip_scalars(self.handle, ctypes.c_void_p(t.data_ptr() if nv else 0), 1, float(threshold), int(flags),
                                                                 out.ctypes.data))
                return self._clip_counts(out)
            scalars = t.numpy()
        a = np.ascontiguousarray(np.asarray(scalars, dtype=np.float64).reshape(-1))
        if len(a) != nv:
            raise ValueError("%d scalars for %d vertices" % (len(a), nv))
        self._check_attr(self.lib.cx_level1_clip_scalars(self.handle, ctypes.c_void_p(a.ctypes.data if nv else 0), 0, float(threshold), int(flags), out.ctypes.data))
        return self._clip_counts(out)

    def level1_clip_field(self, field, value=0.0, flags=0):
        "clip by a second grid sampled at the vertices (cx_level1_sample_grid), the values staying on the device"
        ptr, code, on_dev, keep = self._second_grid(field)
        p = ctypes.c_void_p()
        self._check_attr(self.lib.cx_level1_sample_grid(self.handle, ctypes.c_void_p(ptr), code, on_dev, ctypes.byref(p), None))
        out = np.zeros(8, dtype=np.int64)
        self._check_attr(self.lib.cx_level1_clip_scalars(self.handle, ctypes.c_void_p(p.value or 0), 1, float(value), int(flags), out.ctypes.data))
        del keep
        return self._clip_counts(out)

    def level1_clip_map(self, device=False):
        """(lo_hi (V',2) int32, t (V',) float64): per vertex of the clipped mesh the edge {lo, hi} of the mesh before the clip it lies
        on and where (lo == hi, t == 0: a kept vertex); device=True: torch tensors on the GPU"""
        lp, tp = ctypes.c_void_p(), ctypes.c_void_p()
        self._check_attr(self.lib.cx_level1_clip_map(self.handle, ctypes.byref(lp), ctypes.byref(tp)))      # (none: the library's CX_ERR_STATE)
        nv = self.level1_device_ptrs()[2]
        if device:
            import torch
            return self._device_view(lp.value or 0, (nv, 2), "<i4", torch.int32), self._device_view(tp.value or 0, (nv,), "<f8", torch.float64)
        lo_hi, t = np.zeros((nv, 2), dtype=np.int32), np.zeros(nv, dtype=np.float64)
        self._check_attr(self.lib.cx_level1_clip_map_download(self.handle, lo_hi.ctypes.data if nv else None, t.ctypes.data if nv else None))
        return lo_hi, t

    def level1_clip_info(self):
        "of the last clip: dict(kernels_ms, tail_ms, cut_corners, table_slots, n_vertices_before, n_triangles_before, n_raw_vertices, n_raw_triangles)"
        info = np.zeros(8, dtype=np.float64)
        self._check(self.lib.cx_level1_clip_info(self.handle, info.ctypes.data))
        return dict(kernels_ms=float(info[0]), tail_ms=float(info[1]), cut_corners=int(info[2]), table_slots=int(info[3]), n_vertices_before=int(info[4]),
                    n_triangles_before=int(info[5]), n_raw_vertices=int(info[6]), n_raw_triangles=int(info[7]))

    def surface_geometry(self, points, triangles, do_clean):
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3).copy()
        tris = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3).copy()
        nv = ctypes.c_int64(len(pts))
        nt = ctypes.c_int64(len(tris))
        self._check(self.lib.cx_surface_geometry(self.handle, pts.ctypes.data, ctypes.byref(nv),
                                                 tris.ctypes.data, ctypes.byref(nt), int(bool(do_clean))))
        return pts[:nv.value].copy(), tris[:nt.value].copy()

    # ---- 4-D ---------------------------------------------------------------------------------
    def upload_grid4d(self, array):
        a = np.ascontiguousarray(array, dtype=np.float32)
        assert a.ndim == 4, "4-D sample array expected"
        self._check(self.lib.cx_grid4d_upload(self.handle, a.ctypes.data, *a.shape))
        self.shape4 = tuple(int(n) for n in a.shape)

    def adopt_device_grid4d(self, device_ptr, shape, keepalive=None):
        assert len(shape) == 4
        self._check(self.lib.cx_grid4d_adopt_device(self.handle, ctypes.c_void_p(int(device_ptr)), *[int(n) for n in shape]))
        self.shape4 = tuple(int(n) for n in shape)
        self._keep4 = keepalive

    def extract4d(self, value, flags=CX_DIAG_CPYTHON310):
        c = CxCounts()
        self._check(self.lib.cx_extract4d(self.handle, float(value), int(flags), ctypes.byref(c)))
        return dict(n_cells=c.n_cells, n_vertices=c.n_vertices, n_tetrahedra=c.n_triangles, n_border_voxels=c.n_border_voxels)

    def extract4d_async(self, value, flags=CX_DIAG_CPYTHON310):
        "the 4-D march enqueued on this context's stream, not waited for; counts4d() waits and returns what extract4d returns"
        self._check(self.lib.cx_extract4d_async(self.handle, float(value), int(flags)))

    def counts4d(self):
        c = CxCounts()
        self._check(self.lib.cx_counts4d_get(self.handle, ctypes.byref(c)))
        return dict(n_cells=c.n_cells, n_vertices=c.n_vertices, n_tetrahedra=c.n_triangles, n_border_voxels=c.n_border_voxels)

    def select_seeded4d(self, endpoints, voxel_range=None, all_in_range=False, parallel=False):
        """restrict the 4-D post-pass to the components the reference's seeded search reaches from the lattice end
        point pairs [(i0,j0,k0,l0), (i1,j1,k1,l1)] -> dict(seed_voxels, groups_kept, tetrahedra_kept).
        voxel_range = (lo[4], hi[4]): in_range box of the growth in array coordinates (default: the whole array); seed
        voxels outside it are kept and grow one step into it (an array with a rim around the reference's grid).
        all_in_range: every hyper-voxel inside the box is kept, the end points only add seed voxels outside it."""
        ep = np.ascontiguousarray(np.asarray(endpoints, dtype=np.int64).reshape(-1, 8), dtype=np.int32)
        out = np.zeros(4, dtype=np.int64)
        box = None
        if voxel_range is not None:
            box = np.ascontiguousarray(np.asarray(voxel_range, dtype=np.int64).reshape(8), dtype=np.int32)
        self._check(self.lib.cx_select_seeded4d_ex(self.handle, ep.ctypes.data, int(len(ep)), box.ctypes.data if box is not None else None,
                                                  (1 if all_in_range else 0) | (2 if parallel else 0), out.ctypes.data))
        return dict(seed_voxels=int(out[0]), groups_kept=int(out[1]), tetrahedra_kept=int(out[2]))

    def halo_exchange(self, rccl_comm, rank, world, local_ptr, n_own, plane_samples):
        """send plane 0 of the device buffer to rank-1, receive plane n_own from rank+1 (RCCL, on the context's stream); rccl_comm:
        the caller's ncclComm_t as an integer / ctypes pointer.  (contourist_amd.distributed does this step with torch.distributed.)"""
        self._check(self.lib.cx_halo_exchange(self.handle, rccl_comm, int(rank), int(world), local_ptr, int(n_own), int(plane_samples)))

    def rccl_unique_id(self):
        "128 bytes of a fresh ncclUniqueId (one rank calls this; the bytes go to every rank, e.g. by torch.distributed.broadcast)"
        buf = np.zeros(128, dtype=np.uint8)
        self._check(self.lib.cx_rccl_unique_id(buf.ctypes.data))
        return buf

    def rccl_comm_init(self, id128, rank, world):
        "collective over the ranks: a communicator owned by this context (cx_halo_exchange / slab_step with rccl_comm == NULL)"
        buf = np.ascontiguousarray(id128, dtype=np.uint8)
        assert buf.size == 128
        self._check(self.lib.cx_rccl_comm_init(self.handle, buf.ctypes.data, int(rank), int(world)))

    def rccl_available(self):
        "local, no collective: can this process run the C-side halo exchange (an RCCL copy is loaded and exports what is needed)?"
        return self.lib.cx_rccl_available() == CX_OK

    def rccl_comm_share(self, owner):
        "use `owner`'s communicator (another context of this rank, which keeps the ownership and must outlive this one)"
        self._check(self.lib.cx_rccl_comm_share(self.handle, owner.handle))
        self._comm_owner = owner

    def rccl_comm_destroy(self):
        self._check(self.lib.cx_rccl_comm_destroy(self.handle))
        self._comm_owner = None

    def slab_step(self, local_ptr, n_own, n1, n2, rank, world, value, flags=CX_DIAG_CPYTHON310, keepalive=None):
        """one rank's whole step for one volume in ONE call: adopt the device buffer (n_own planes + room for the halo plane unless
        this is the last rank), halo exchange on this context's stream with its own communicator, extraction enqueued behind it"""
        self._check(self.lib.cx_slab_step(self.handle, ctypes.c_void_p(int(local_ptr)), int(n_own), int(n1), int(n2), int(rank), int(world),
                                          float(value), int(flags)))
        self.shape = (int(n_own) + (1 if rank + 1 < world else 0), int(n1), int(n2))
        self._keep = keepalive

    def seeded_mode(self):
        "how the last seeded selection ran its end points: 'sequential' (the reference's shared visited set) or 'parallel'"
        m = ctypes.c_int(0)
        self._check(self.lib.cx_seeded_mode(self.handle, ctypes.byref(m)))
        return "parallel" if m.value else "sequential"

    def seeded4d_mask(self, counts):
        "mask over the Level-0 tetrahedra left by select_seeded4d (uint8, 1 = kept)"
        keep = np.zeros(int(counts["n_tetrahedra"]), dtype=np.uint8)
        self._check(self.lib.cx_seeded4d_mask_download(self.handle, keep.ctypes.data))
        return keep

    def download_level0_4d(self, counts):
        "-> (xyzt (V,4) float32, edge ids (V,) uint32, tetrahedra (T,4) int32)"
        nv, nt = int(counts["n_vertices"]), int(counts["n_tetrahedra"])
        verts = np.empty((nv, 4), dtype=np.float32)
        keys = np.empty(nv, dtype=np.uint32)
        tets = np.empty((nt, 4), dtype=np.int32)
        self._check(self.lib.cx_level0_4d_download(self.handle, verts.ctypes.data, keys.ctypes.data, tets.ctypes.data))
        return verts, keys, tets

    def postprocess4d(self, nbins=100, points=None):
        """bin_times / drop_instant / tiny collapse on the device; points: (n_vertices, 4) float64 replacing the linearly
        interpolated crossing points (linear_interpolate=False: refined on the host), in the reference's lattice"""
        out = np.zeros(8, dtype=np.int64)
        if points is not None:
            pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 4)
            self._check(self.lib.cx_postprocess4d_points(self.handle, int(nbins), pts.ctypes.data, out.ctypes.data))
        else:
            self._check(self.lib.cx_postprocess4d(self.handle, int(nbins), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_tetrahedra=int(out[1]), n_after_drop=int(out[2]), n_after_tiny=int(out[3]))

    def download_level1_4d(self, counts):
        pts = np.empty((int(counts["n_vertices"]), 4), dtype=np.float64)
        tets = np.empty((int(counts["n_tetrahedra"]), 4), dtype=np.int32)
        self._check(self.lib.cx_level1_4d_download(self.handle, pts.ctypes.data, tets.ctypes.data))
        return pts, tets

    # -- a 4-D volume of more than one extraction, slab by slab (cx_slab4d_*) --------------------------------------------
    def slab4d_begin(self, whole_shape):
        "start the assembly of a volume of shape whole_shape (n0, n1, n2, n3), marched slab by slab along axis 0"
        shape = np.ascontiguousarray([int(n) for n in whole_shape], dtype=np.int64)
        assert shape.shape == (4,)
        self._check(self.lib.cx_slab4d_begin(self.handle, shape.ctypes.data))

    def slab4d_append(self, i0, owned_planes):
        """append the slab just marched (extract4d with set_origin4d(i0, 0, 0, 0)): planes i0 .. i0 + owned_planes of the whole volume,
        the bound array holding one more (the halo) unless it is the last slab"""
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_slab4d_append(self.handle, int(i0), int(owned_planes), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_tetrahedra=int(out[1]), slab_vertices=int(out[2]), slab_tetrahedra=int(out[3]),
                    pending=int(out[4]), n_slabs=int(out[5]))

    def slab4d_finish(self, nbins=100):
        "the post-steps of postprocess4d on the assembly; returns what postprocess4d returns (download_level1_4d, morph_triangles follow)"
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_slab4d_finish(self.handle, int(nbins), out.ctypes.data))
        return dict(n_vertices=int(out[0]), n_tetrahedra=int(out[1]), n_after_drop=int(out[2]), n_after_tiny=int(out[3]))

    def slab4d_keys(self, counts):
        "global edge id (int64) of every assembled vertex, in the order of the points"
        keys = np.empty(int(counts["n_vertices"]), dtype=np.int64)
        self._check(self.lib.cx_slab4d_download_keys(self.handle, keys.ctypes.data))
        return keys

    def morph_triangles(self):
        "-> (points4d (V,4) float64, segments (S,2) int32 low t -> high t, triangles (T,3) int32 oriented)"
        out = np.zeros(8, dtype=np.int64)
        self._check(self.lib.cx_morph_triangles(self.handle, out.ctypes.data))
        pts = np.empty((int(out[0]), 4), dtype=np.float64)
        segs = np.empty((int(out[1]), 2), dtype=np.int32)
        tris = np.empty((int(out[2]), 3), dtype=np.int32)
        self._check(self.lib.cx_morph_download(self.handle, pts.ctypes.data, segs.ctypes.data, tris.ctypes.data))
        return pts, segs, tris, int(out[4])

    def morph_eval(self, t, download=True):
        """surface at time t from the last morph_triangles() -> (points (P,3) float64, triangles (Q,3) int32)
        or, with download=False, just the counts (the mesh stays on the device)"""
        out = np.zeros(2, dtype=np.int64)
        self._check(self.lib.cx_morph_eval(self.handle, float(t), out.ctypes.data))
        if not download:
            return int(out[0]), int(out[1])
        pts = np.empty((int(out[0]), 3), dtype=np.float64)
        tris = np.empty((int(out[1]), 3), dtype=np.int32)
        self._check(self.lib.cx_morph_eval_download(self.handle, pts.ctypes.data, tris.ctypes.data))
        return pts, tris

    def morph_eval_many(self, times, download=True, out=None):
        """the surfaces at all `times` from the last morph_triangles() in one set of launches (cx_morph_eval_many)
        -> list of (points (P,3) float64, triangles (Q,3) int32), one per time, each what morph_eval(t) returns;
        with download=False the counts array (n,2) int64 (the meshes stay on the device: morph_eval_device_ptrs(i)).
        out = (points (>= sum P, 3) float64, triangles (>= sum Q, 3) int32): arrays to download into (a consumer that plays stream
        after stream keeps them: fresh arrays cost their page faults, ~20 ms for the 428 MB of config 4's 64 surfaces against 11 ms)"""
        _out = out
        ts = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        out = np.zeros((len(ts), 2), dtype=np.int64)
        self._check(self.lib.cx_morph_eval_many(self.handle, ts.ctypes.data, len(ts), out.ctypes.data))
        if not download:
            return out
        # one transfer for all surfaces (cx_morph_eval_many_download_all); the surfaces are views into the two arrays
        counts = out
        npts, ntri = int(counts[:, 0].sum()), int(counts[:, 1].sum())
        pts_all = tris_all = None
        if _out is not None:
            pts_all, tris_all = _out
            ok = (pts_all.dtype == np.float64 and tris_all.dtype == np.int32 and pts_all.flags.c_contiguous and tris_all.flags.c_contiguous
                  and pts_all.ndim == 2 and tris_all.ndim == 2 and pts_all.shape[1] == 3 and tris_all.shape[1] == 3
                  and len(pts_all) >= npts and len(tris_all) >= ntri)
            if not ok:
                raise ValueError("out: C-contiguous (>= %d, 3) float64 and (>= %d, 3) int32 arrays expected" % (npts, ntri))
        else:
            pts_all = np.empty((npts, 3), dtype=np.float64)
            tris_all = np.empty((ntri, 3), dtype=np.int32)
        self._check(self.lib.cx_morph_eval_many_download_all(self.handle, pts_all.ctypes.data, tris_all.ctypes.data))
        res, p0, t0 = [], 0, 0
        for i in range(len(ts)):
            npi, nti = int(out[i, 0]), int(out[i, 1])
            res.append((pts_all[p0:p0 + npi], tris_all[t0:t0 + nti]))
            p0 += npi; t0 += nti
        return res

    def morph_eval_device_ptrs(self, i):
        "device addresses (points float64 x 3, triangles int32 x 3) of surface i of the last morph_eval_many / morph_eval; 0 for an empty one"
        p, t = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self.lib.cx_morph_eval_many_device_ptrs(self.handle, int(i), ctypes.byref(p), ctypes.byref(t)))
        return int(p.value or 0), int(t.value or 0)

    def contour2d(self, samples, values, seeds=None, flags=0, mins_delta=None, device_ptr=None, shape=None):
        """polylines of a 2-D sample array at every isovalue of `values` (ascending, distinct)
        -> (points (P,2) float64, keys (P,) int64, chains (C,) CHAIN2D_DTYPE, n_pairs).
        samples: fp32 numpy array (n, m), or None with device_ptr + shape for samples already in HBM.
        seeds: (S,4) int32 rows (i, j, role, level index), or None for the reference's grid search."""
        vals = np.ascontiguousarray(values, dtype=np.float64)
        if device_ptr is None:
            arr = np.ascontiguousarray(samples, dtype=np.float32)
            assert arr.ndim == 2
            n, m = arr.shape
            ptr, on_device = arr.ctypes.data, 0
        else:
            n, m = (int(x) for x in shape)
            ptr, on_device = int(device_ptr), 1
        sd = None if seeds is None else np.ascontiguousarray(seeds, dtype=np.int32).reshape(-1, 4)
        md = None if mins_delta is None else np.ascontiguousarray(mins_delta, dtype=np.float64).reshape(4)
        c = CxCounts2D()
        self._check(self.lib.cx_contour2d_extract(self.handle, ptr, on_device, n, m, vals.ctypes.data, len(vals),
                                                  None if sd is None or len(sd) == 0 else sd.ctypes.data, 0 if sd is None else len(sd),
                                                  int(flags), None if md is None else md.ctypes.data, ctypes.byref(c)))
        pts = np.empty((c.n_points, 2), dtype=np.float64)
        keys = np.empty((c.n_points,), dtype=np.int64)
        chains = np.empty((c.n_chains,), dtype=CHAIN2D_DTYPE)
        self._check(self.lib.cx_contour2d_download(self.handle, pts.ctypes.data, keys.ctypes.data, chains.ctypes.data))
        return pts, keys, chains, int(c.n_pairs)

    # what cx_timing_read's slots measure, with the algorithmic bytes of each stage (bench.py)
    def level0_path(self):
        "kernels of the last extraction: 0 generic classify + triangle stage, 1 staged pipeline, 2 stream + scan + fused emit, 3 stream + scan + tile emit + boundary"
        p = ctypes.c_int()
        self._check(self.lib.cx_level0_path(self.handle, ctypes.byref(p)))
        return p.value

    def kernel_names(self):
        path = self.level0_path()
        if path == 2:
            return [("stream_ms", "cx_k_stream"), ("scan_ms", "cx_k_scan_list"), ("cells_ms", "cx_k_cell_info+cx_k_emit_mesh")]
        if path == 1:
            return [("stream_ms", "cx_k_stream"), ("scan_ms", "cx_k_scan_list"),
                    ("cells_ms", "cx_k_emit_vertices"), ("emit_ms", "cx_k_emit_triangles_q")]
        if path == 3:
            return [("stream_ms", "cx_k_stream"), ("scan_ms", "cx_k_scan_list"),
                    ("cells_ms", "cx_k_tile_emit"), ("emit_ms", "cx_k_tile_boundary")]
        return [("stream_ms", "cx_k_classify_generic"), ("emit_ms", "cx_k_emit_triangles")]

    def vertex_stage_bytes(self, counts):
        if self.level0_path() in (2, 3):     # fused emit / tile emit: 8 B per vertex record + 12 B per triangle written by ONE kernel
            return 8.0 * counts["n_vertices"] + 12.0 * counts["n_triangles"]
        # what the stage must leave: 8-byte vertex records.  (Its cell records and per-entry words are the pipeline's own
        # intermediates -- traffic, not algorithmic bytes.)
        return 8.0 * counts["n_vertices"]

    def triangle_stage_bytes(self, counts):
        if self.level0_path() == 3:          # the boundary kernel: the triangles of ~13 % of the voxels (counted with the tile kernel above)
            return 0.0
        return 12.0 * counts["n_triangles"]

    def measure_read_bandwidth(self, device_ptr, nbytes, reps=5):
        "GB/s of a plain streaming read of nbytes at device_ptr (best of reps launches)"
        g = ctypes.c_double()
        self._check(self.lib.cx_measure_read_bandwidth(self.handle, ctypes.c_void_p(int(device_ptr)), int(nbytes), int(reps), ctypes.byref(g)))
        return g.value

    def timing_enable(self, on=True):
        self._check(self.lib.cx_timing_enable(self.handle, int(bool(on))))

    def timing_read(self):
        ms = (ctypes.c_double * 8)()
        n = ctypes.c_int()
        self._check(self.lib.cx_timing_read(self.handle, ms, ctypes.byref(n)))
        return dict(classify_ms=ms[0], emit_ms=ms[1], total_ms=ms[2], stream_ms=ms[3], scan_ms=ms[4],
                    cells_ms=ms[5], n=n.value)
