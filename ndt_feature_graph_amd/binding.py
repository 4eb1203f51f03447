"""ctypes host layer over libndtgpu.so (include/ndtgpu.h)."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
_SO = os.path.join(_HERE, "libndtgpu.so")
_SOURCES = ["ndt_build.hip", "ndt_build_flat.hip", "ndt_match.hip", "ndt_fuse.hip", "ndt_pack.hip", "ndt_fuser.hip", "ndtgpu_api.hip",
            "ndtgpu_matcher.hip", "ndtgpu_registrar.hip", "ndtgpu_fuser_bank.hip", "ndt_multires.hip", "ndtgpu_multires.hip",
            "ndt_mcl.hip", "ndtgpu_mcl.hip", "ndt_pgo.hip", "ndt_pgo_wide.hip", "ndtgpu_pgo.hip", "ndt_pgo3.hip", "ndt_pgo3_wide.hip", "ndtgpu_pgo3.hip",
            "ndt_pgo_robust.hip", "ndtgpu_pgo_robust.hip", "ndt_featmatch.hip", "ndtgpu_featmatch.hip",
            "ndt_featextract.hip", "ndt_world.hip", "ndtgpu_world.hip", "ndt_occgrid.hip", "ndtgpu_occgrid.hip", "ndt_linkgate.hip",
            "ndtgpu_linkgate.hip", "ndt_fuserfeat.hip", "ndt_scanproject.hip", "ndtgpu_scanproject.hip",
            "ndt_calib.hip", "ndtgpu_calib.hip", "ndt_locmon.hip", "ndtgpu_locmon.hip", "ndt_scansim.hip", "ndtgpu_scansim.hip",
            "ndt_marker.hip", "ndtgpu_marker.hip"]

STATUS = {0: "OK", -1: "ERR_INVALID", -2: "ERR_HIP", -3: "ERR_NO_DEVICE", -4: "ERR_CAPACITY", -5: "ERR_ALLOC"}


class NdtGpuError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("ndtgpu %s (%d): %s" % (STATUS.get(status, "?"), status, msg))
        self.status = status


def library_path():
    """The in-tree library; NDTGPU_LIB names another build of it (A/B measurements of kernel variants)."""
    return os.environ.get("NDTGPU_LIB") or _SO


# per-source flags.  ndt_match.hip: the solver's pivoted LDL^T picks one of several statically indexed register swaps; with
# common-code sinking the optimiser merges those branches into ONE swap with computed indices, and the register array
# goes to the stack (the only private segment the matcher kernels would have).
# ndt_build_flat.hip: the same pass merges the two symmetric "replace run A / run B" branches into one that works through a
# POINTER to the run's scalar state, which then lives in scratch memory instead of scalar registers.
# ndt_build.hip: the same for the two runs of a lane in the 3D (SCAT) point loop -- their second moments were 112 B of
# scratch per lane and a memory round trip per point until round 4.
_SOURCE_FLAGS = {"ndt_match.hip": ["-mllvm", "-simplifycfg-sink-common=false"],
                 "ndt_build_flat.hip": ["-mllvm", "-simplifycfg-sink-common=false"],
                 "ndt_build.hip": ["-mllvm", "-simplifycfg-sink-common=false"]}


def build_library(force=False, verbose=False):
    """hipcc cross-compiles the kernels + C-ABI for gfx950 into the in-tree libndtgpu.so (one object per source, in
    parallel, then one link)."""
    csrc = os.path.join(_HERE, "csrc")
    so = library_path()
    srcs = [os.path.join(csrc, s) for s in _SOURCES]
    deps = srcs + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(_ROOT, "include", "ndtgpu.h"), os.path.abspath(__file__)]
    if not force and os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(d) for d in deps):
        return so
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        hipcc = "hipcc"
    extra = os.environ.get("NDTGPU_BUILD_FLAGS", "").split()      # experiments only (-DNDT_MATCH_PROF ...)
    # one object directory per output library: concurrent builds of variants (tools/build_variant.sh) do not share objects
    tag = os.path.splitext(os.path.basename(so))[0]
    objdir = os.path.join(_HERE, "build") if so == _SO else os.path.join(_HERE, "build", tag)
    os.makedirs(objdir, exist_ok=True)
    # (spills never go to AGPRs: with AGPRs in use the matcher kernel would not keep 256 architectural VGPRs at two
    #  waves per SIMD)
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-bitwise-instead-of-logical",
              "-mllvm", "-amdgpu-spill-vgpr-to-agpr=0", *extra]
    jobs = []
    for name, src in zip(_SOURCES, srcs):
        obj = os.path.join(objdir, name + ".o")
        cmd = common + _SOURCE_FLAGS.get(name, []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        jobs.append((subprocess.Popen(cmd), cmd, obj))
    objs, failed = [], None
    for proc, cmd, obj in jobs:                 # every compile job is reaped, also after a failure
        if proc.wait() != 0 and failed is None:
            failed = (proc.returncode, cmd)
        objs.append(obj)
    if failed:
        raise subprocess.CalledProcessError(*failed)
    link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", so + ".tmp"]
    if verbose:
        print(" ".join(link))
    subprocess.check_call(link)
    os.replace(so + ".tmp", so)
    return so


class GridParams(C.Structure):
    _fields_ = [("res", C.c_double), ("centre", C.c_double * 3), ("size", C.c_double * 3), ("max_cells", C.c_uint32)]


class CellParams(C.Structure):
    _fields_ = [("n_min", C.c_int32), ("eval_factor", C.c_double)]


class FuseParams(C.Structure):
    _fields_ = [("maxz", C.c_double), ("sensor_noise", C.c_double), ("maxnumpoints", C.c_double),
                ("occupancy_limit", C.c_double), ("n_min", C.c_int32), ("eval_factor", C.c_double)]


class MatchParams(C.Structure):
    _fields_ = [("n_neighbours", C.c_int32), ("itr_max", C.c_int32), ("delta_score", C.c_double),
                ("step_control", C.c_int32), ("lfd1", C.c_double), ("lfd2", C.c_double), ("dof_mask", C.c_int32),
                ("use_initial_guess", C.c_int32)]


class MatchResult(C.Structure):
    _fields_ = [("converged", C.c_int32), ("iterations", C.c_int32), ("fevals", C.c_int32), ("exit_code", C.c_int32),
                ("score", C.c_double), ("n_source", C.c_int32), ("n_target", C.c_int32),
                ("cycles_eval", C.c_int64), ("cycles_solver", C.c_int64),
                ("pair_terms_g", C.c_int64), ("pair_terms_h", C.c_int64)]


class CalibParams(C.Structure):
    _fields_ = [("max_dist", C.c_double)]


class CalibResult(C.Structure):
    _fields_ = [("score", C.c_double), ("index", C.c_uint32), ("flags", C.c_uint32), ("n_skipped", C.c_uint32), ("reserved", C.c_uint32)]


class LocmonParams(C.Structure):
    _fields_ = [("max_dist", C.c_double), ("r_min", C.c_double), ("r_max", C.c_double), ("post_x", C.c_double), ("post_y", C.c_double),
                ("occupied_min", C.c_int32), ("min_num_matches", C.c_int32)]


class LocmonQuery(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("c", C.c_double), ("s", C.c_double), ("scan", C.c_uint32), ("grid", C.c_uint32)]


class LocmonResult(C.Structure):
    _fields_ = [("badness", C.c_double), ("key", C.c_uint32), ("n_kept", C.c_uint32), ("n_offmap", C.c_uint32), ("flags", C.c_uint32)]


class LocmonAdjustResult(C.Structure):
    _fields_ = [("badness", C.c_double), ("key", C.c_uint32), ("index", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class LocmonPick(C.Structure):
    _fields_ = [("pair", C.c_int32), ("n_inliers", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


LOCMON_QUERY_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("c", "<f8"), ("s", "<f8"), ("scan", "<u4"), ("grid", "<u4")])
LOCMON_RESULT_DTYPE = np.dtype([("badness", "<f8"), ("key", "<u4"), ("n_kept", "<u4"), ("n_offmap", "<u4"), ("flags", "<u4")])
LOCMON_ADJUST_DTYPE = np.dtype([("badness", "<f8"), ("key", "<u4"), ("index", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
LOCMON_PICK_DTYPE = np.dtype([("pair", "<i4"), ("n_inliers", "<i4"), ("flags", "<u4"), ("reserved", "<u4")])
assert LOCMON_QUERY_DTYPE.itemsize == C.sizeof(LocmonQuery) == 40 and LOCMON_RESULT_DTYPE.itemsize == C.sizeof(LocmonResult) == 24
assert LOCMON_ADJUST_DTYPE.itemsize == C.sizeof(LocmonAdjustResult) == 24 and LOCMON_PICK_DTYPE.itemsize == C.sizeof(LocmonPick) == 16

class ScansimParams(C.Structure):
    _fields_ = [("range_max", C.c_double), ("miss", C.c_double), ("occupied_min", C.c_int32), ("unknown_is_obstacle", C.c_int32)]


class ScansimResult(C.Structure):
    _fields_ = [("n_hits", C.c_uint32), ("flags", C.c_uint32)]


class MarkerParams(C.Structure):
    _fields_ = [("min_eval", C.c_double), ("particle_length", C.c_double), ("skip_negative", C.c_int32), ("reserved", C.c_int32)]


assert C.sizeof(MarkerParams) == 24

SCANSIM_RESULT_DTYPE = np.dtype([("n_hits", "<u4"), ("flags", "<u4")])
assert SCANSIM_RESULT_DTYPE.itemsize == C.sizeof(ScansimResult) == 8 and C.sizeof(ScansimParams) == 24

CALIB_RESULT_DTYPE = np.dtype([("score", "<f8"), ("index", "<u4"), ("flags", "<u4"), ("n_skipped", "<u4"), ("reserved", "<u4")])
assert CALIB_RESULT_DTYPE.itemsize == C.sizeof(CalibResult) == 24

RESULT_DTYPE = np.dtype([("converged", "<i4"), ("iterations", "<i4"), ("fevals", "<i4"), ("exit_code", "<i4"),
                         ("score", "<f8"), ("n_source", "<i4"), ("n_target", "<i4"), ("cycles_eval", "<i8"),
                         ("cycles_solver", "<i8"), ("pair_terms_g", "<i8"), ("pair_terms_h", "<i8")])
assert RESULT_DTYPE.itemsize == C.sizeof(MatchResult)

# every symbol include/ndtgpu.h declares (checked by tests/test_abi.py against the header text)
EXPORTS = ["ndtgpu_version", "ndtgpu_last_error", "ndtgpu_device_count", "ndtgpu_default_cell_params",
           "ndtgpu_default_match_params", "ndtgpu_mapset_create", "ndtgpu_mapset_destroy", "ndtgpu_mapset_set_centre",
           "ndtgpu_mapset_info", "ndtgpu_mapset_build", "ndtgpu_mapset_build_host", "ndtgpu_mapset_num_cells",
           "ndtgpu_mapset_export_cells", "ndtgpu_mapset_set_cells", "ndtgpu_derivatives", "ndtgpu_match_batch",
           "ndtgpu_match_batch_device", "ndtgpu_match_d2d", "ndtgpu_kernel_name", "ndtgpu_profiling_enable",
           "ndtgpu_last_kernel_ms", "ndtgpu_mapset_counters", "ndtgpu_match_fusion_batch",
           "ndtgpu_mapset_enable_occupancy", "ndtgpu_default_fuse_params", "ndtgpu_mapset_add_cloud",
           "ndtgpu_mapset_add_cloud_host", "ndtgpu_mapset_clear", "ndtgpu_mapset_export_occupancy",
           "ndtgpu_overlap_score_batch", "ndtgpu_covariance_batch", "ndtgpu_mapset_discard_cells", "ndtgpu_mapset_import_occupancy",
           "ndtgpu_match_fusion_feat_batch", "ndtgpu_match_aborted", "ndtgpu_mapset_pack_bytes",
           "ndtgpu_mapset_pack_cells_device", "ndtgpu_mapset_unpack_cells_device", "ndtgpu_mapset_pack_bytes_sparse",
           "ndtgpu_mapset_occupied_cells_max", "ndtgpu_mapset_pack_cells_sparse_device", "ndtgpu_mapset_build_host_async",
           "ndtgpu_mapset_add_cloud_host_async", "ndtgpu_registrar_create", "ndtgpu_registrar_destroy",
           "ndtgpu_register_batch_device", "ndtgpu_registrar_wait_stream", "ndtgpu_registrar_sync",
           "ndtgpu_registrar_profiling", "ndtgpu_registrar_kernel_ms", "ndtgpu_registrar_mapset", "ndtgpu_register_batch_host",
           "ndtgpu_default_registrar_params", "ndtgpu_registrar_create_ex", "ndtgpu_registrar_get_info",
           "ndtgpu_default_fuser_params", "ndtgpu_fuser_prepare", "ndtgpu_fuser_bank_create", "ndtgpu_fuser_bank_destroy",
           "ndtgpu_fuser_bank_mapsets", "ndtgpu_fuser_initialize_batch", "ndtgpu_fuser_update_batch", "ndtgpu_fuser_poses",
           "ndtgpu_fuser_initialize_batch_host", "ndtgpu_fuser_update_batch_host", "ndtgpu_registrar_inject_abort",
           "ndtgpu_register_batch_cov_device", "ndtgpu_register_batch_cov_host", "ndtgpu_default_resolutions",
           "ndtgpu_multires_create", "ndtgpu_multires_destroy", "ndtgpu_register_multires_device", "ndtgpu_register_multires_host",
           "ndtgpu_multires_get_info", "ndtgpu_default_mcl_params", "ndtgpu_mcl_create", "ndtgpu_mcl_destroy", "ndtgpu_mcl_initialize",
           "ndtgpu_mcl_set_particles", "ndtgpu_mcl_update", "ndtgpu_mcl_update_host", "ndtgpu_mcl_particles", "ndtgpu_mcl_mean",
           "ndtgpu_default_pgo_params", "ndtgpu_pgo_create", "ndtgpu_pgo_destroy", "ndtgpu_pgo_set_graph", "ndtgpu_pgo_set_links_device",
           "ndtgpu_pgo_optimize", "ndtgpu_pgo_poses", "ndtgpu_live_resources",
           "ndtgpu_default_pgo_wide_params", "ndtgpu_pgo_wide_plan", "ndtgpu_pgo_optimize_wide",
           "ndtgpu_default_pgo3_params", "ndtgpu_pgo3_create", "ndtgpu_pgo3_destroy", "ndtgpu_pgo3_set_graph",
           "ndtgpu_pgo3_set_links_device", "ndtgpu_pgo3_optimize", "ndtgpu_pgo3_poses", "ndtgpu_pgo3_link_error", "ndtgpu_pgo3_retract",
           "ndtgpu_pgo3_link_from_registration", "ndtgpu_pgo3_wide_plan", "ndtgpu_pgo3_optimize_wide",
           "ndtgpu_default_pgo_marginal_params", "ndtgpu_pgo_marginal_plan", "ndtgpu_pgo_marginals", "ndtgpu_pgo_marginals_device",
           "ndtgpu_pgo3_marginals", "ndtgpu_pgo3_marginals_device", "ndtgpu_pgo_relative_covariance", "ndtgpu_pgo3_relative_covariance",
           "ndtgpu_default_pgo_robust_params", "ndtgpu_pgo_robust_weight", "ndtgpu_pgo_optimize_robust", "ndtgpu_pgo3_optimize_robust",
           "ndtgpu_pgo_robust_links", "ndtgpu_pgo3_robust_links", "ndtgpu_pgo_robust_links_device", "ndtgpu_pgo3_robust_links_device",
           "ndtgpu_pgo_robust_restore", "ndtgpu_pgo3_robust_restore", "ndtgpu_pgo_link_information", "ndtgpu_pgo3_link_information",
           "ndtgpu_default_featmatch_params", "ndtgpu_featbank_create", "ndtgpu_featbank_destroy", "ndtgpu_featbank_set",
           "ndtgpu_featbank_match", "ndtgpu_featbank_match_device", "ndtgpu_featbank_results",
           "ndtgpu_default_featextract_params", "ndtgpu_featbank_extract", "ndtgpu_featbank_extract_device",
           "ndtgpu_featbank_extract_results", "ndtgpu_featbank_get",
           "ndtgpu_default_world_params", "ndtgpu_world_assemble", "ndtgpu_world_check",
           "ndtgpu_default_occgrid_params", "ndtgpu_occgrid_dims", "ndtgpu_mapset_occupancy_grid_device", "ndtgpu_mapset_occupancy_grid",
           "ndtgpu_occgrid_move", "ndtgpu_occgrid_check",
           "ndtgpu_default_linkgate_params", "ndtgpu_linkgate_check", "ndtgpu_linkgate_create", "ndtgpu_linkgate_destroy",
           "ndtgpu_linkgate_set_nodes", "ndtgpu_linkgate_set_nodes_device", "ndtgpu_linkgate_candidates", "ndtgpu_linkgate_valid",
           "ndtgpu_linkgate_gather", "ndtgpu_linkgate_count", "ndtgpu_linkgate_keep", "ndtgpu_linkgate_candidates_host",
           "ndtgpu_linkgate_valid_host",
           "ndtgpu_default_fuser_feat_params", "ndtgpu_fuser_feat_prepare", "ndtgpu_fuser_feat_move", "ndtgpu_fuser_bank_attach_features",
           "ndtgpu_fuser_initialize_batch_feat", "ndtgpu_fuser_update_batch_feat", "ndtgpu_fuser_feat_results", "ndtgpu_fuser_feat_cells",
           "ndtgpu_fuser_initialize_batch_feat_host", "ndtgpu_fuser_update_batch_feat_host",
           "ndtgpu_default_scanproject_params", "ndtgpu_scanproj_tile", "ndtgpu_scanproj_check", "ndtgpu_scanproj_beam",
           "ndtgpu_scanproj_create", "ndtgpu_scanproj_destroy", "ndtgpu_scanproj_project_device", "ndtgpu_scanproj_project",
           "ndtgpu_default_calib_params", "ndtgpu_calib_tile", "ndtgpu_calib_lattice", "ndtgpu_calib_pair_motion", "ndtgpu_calib_select_pairs",
           "ndtgpu_calib_check", "ndtgpu_calib_create", "ndtgpu_calib_destroy", "ndtgpu_calib_search_device", "ndtgpu_calib_search",
           "ndtgpu_default_locmon_params", "ndtgpu_locmon_tile", "ndtgpu_locmon_check", "ndtgpu_locmon_radius", "ndtgpu_locmon_beam_table",
           "ndtgpu_locmon_pixel", "ndtgpu_locmon_metres", "ndtgpu_locmon_compose", "ndtgpu_locmon_create", "ndtgpu_locmon_destroy",
           "ndtgpu_locmon_set_beams", "ndtgpu_locmon_set_grids_device", "ndtgpu_locmon_set_grids", "ndtgpu_locmon_field_get",
           "ndtgpu_locmon_evaluate_device", "ndtgpu_locmon_evaluate", "ndtgpu_locmon_adjust_device", "ndtgpu_locmon_adjust",
           "ndtgpu_locmon_pick_device",
           "ndtgpu_default_scansim_params", "ndtgpu_scansim_tile", "ndtgpu_scansim_check", "ndtgpu_scansim_reach", "ndtgpu_scansim_skip",
           "ndtgpu_scansim_cell", "ndtgpu_scansim_beam", "ndtgpu_scansim_headings", "ndtgpu_scansim_create", "ndtgpu_scansim_destroy",
           "ndtgpu_scansim_set_beams", "ndtgpu_scansim_set_grids_device", "ndtgpu_scansim_set_grids", "ndtgpu_scansim_lattice_device",
           "ndtgpu_scansim_lattice", "ndtgpu_scansim_simulate_device", "ndtgpu_scansim_simulate",
           "ndtgpu_default_marker_params", "ndtgpu_marker_tile", "ndtgpu_marker_check", "ndtgpu_marker_eig3", "ndtgpu_marker_cell",
           "ndtgpu_marker_create", "ndtgpu_marker_destroy", "ndtgpu_mapset_markers_device", "ndtgpu_mapset_markers", "ndtgpu_marker_count",
           "ndtgpu_marker_links_device", "ndtgpu_marker_links", "ndtgpu_mcl_markers_device", "ndtgpu_mcl_markers"]

_lib = None


def lib():
    """Loads libndtgpu.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # PyTorch bundles its own libamdhip64.so.7; load it first so that ONE HIP runtime serves both
        # torch (device memory, streams, torch.distributed) and libndtgpu.so (same soname -> shared).
        import torch  # noqa: F401
    except ImportError:
        pass
    so = library_path()
    if not os.path.exists(so):
        raise NdtGpuError(-2, "HIP extension %s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % so)
    L = C.CDLL(so)
    vp, dp, u32p, i32p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    L.ndtgpu_version.restype = C.c_char_p
    L.ndtgpu_last_error.restype = C.c_char_p
    L.ndtgpu_kernel_name.restype = C.c_char_p
    L.ndtgpu_kernel_name.argtypes = [C.c_int]
    L.ndtgpu_device_count.restype = C.c_int
    L.ndtgpu_default_cell_params.argtypes = [C.POINTER(CellParams)]
    L.ndtgpu_default_match_params.argtypes = [C.POINTER(MatchParams)]
    L.ndtgpu_mapset_create.argtypes = [C.POINTER(GridParams), C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_mapset_destroy.argtypes = [vp]
    L.ndtgpu_mapset_set_centre.argtypes = [vp, C.c_size_t, dp]
    L.ndtgpu_mapset_info.argtypes = [vp, C.POINTER(C.c_size_t), i32p, u32p]
    L.ndtgpu_mapset_build.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double,
                                      dp, C.POINTER(CellParams), vp]
    L.ndtgpu_mapset_build_host.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_double, dp, C.POINTER(CellParams)]
    L.ndtgpu_mapset_build_host_async.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 C.c_double, dp, C.POINTER(CellParams), vp]
    L.ndtgpu_mapset_num_cells.argtypes = [vp, C.c_size_t, u32p]
    L.ndtgpu_mapset_export_cells.argtypes = [vp, C.c_size_t, dp, dp, i32p, u32p]
    L.ndtgpu_mapset_set_cells.argtypes = [vp, C.c_size_t, dp, dp, C.c_size_t]
    L.ndtgpu_derivatives.argtypes = [vp, C.c_size_t, dp, dp, C.c_size_t, C.c_int, C.c_int, C.c_double, C.c_double,
                                     dp, dp, dp]
    L.ndtgpu_match_batch.argtypes = [vp, u32p, vp, u32p, dp, C.c_size_t, C.POINTER(MatchParams), vp, vp]
    L.ndtgpu_match_fusion_batch.argtypes = [vp, u32p, vp, u32p, dp, dp, C.c_size_t, C.POINTER(MatchParams), C.c_int, vp, vp]
    L.ndtgpu_match_batch_device.argtypes = [vp, vp, vp, vp, vp, C.c_size_t, C.POINTER(MatchParams), vp, vp]
    L.ndtgpu_match_d2d.argtypes = [vp, C.c_size_t, vp, C.c_size_t, dp, C.POINTER(MatchParams), C.POINTER(MatchResult)]
    L.ndtgpu_profiling_enable.argtypes = [vp, C.c_int]
    L.ndtgpu_last_kernel_ms.argtypes = [vp, C.c_int, C.POINTER(C.c_float)]
    L.ndtgpu_mapset_counters.argtypes = [vp, C.c_size_t, u32p]
    L.ndtgpu_mapset_enable_occupancy.argtypes = [vp]
    L.ndtgpu_default_fuse_params.argtypes = [C.POINTER(FuseParams)]
    L.ndtgpu_mapset_add_cloud.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, dp,
                                          C.POINTER(FuseParams), vp]
    L.ndtgpu_mapset_add_cloud_host.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, dp,
                                               C.POINTER(FuseParams)]
    L.ndtgpu_mapset_add_cloud_host_async.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t, dp,
                                                     C.POINTER(FuseParams), vp]
    L.ndtgpu_mapset_clear.argtypes = [vp, C.c_size_t, C.c_size_t]
    L.ndtgpu_mapset_export_occupancy.argtypes = [vp, C.c_size_t, C.POINTER(C.c_float)]
    L.ndtgpu_overlap_score_batch.argtypes = [vp, u32p, vp, u32p, dp, C.c_size_t, dp, C.POINTER(C.c_int64), vp]
    L.ndtgpu_mapset_import_occupancy.argtypes = [vp, C.c_size_t, C.POINTER(C.c_float)]
    L.ndtgpu_mapset_discard_cells.argtypes = [vp, C.c_size_t, C.POINTER(C.c_float), C.c_size_t]
    L.ndtgpu_covariance_batch.argtypes = [vp, u32p, vp, u32p, dp, C.c_size_t, C.POINTER(MatchParams), C.c_int, dp, i32p, vp]
    L.ndtgpu_match_aborted.argtypes = [vp, i32p]
    L.ndtgpu_mapset_pack_bytes.restype = C.c_size_t
    L.ndtgpu_mapset_pack_bytes.argtypes = [vp, C.c_uint32, C.c_int]
    L.ndtgpu_mapset_pack_cells_device.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_int, vp]
    L.ndtgpu_mapset_unpack_cells_device.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_int, vp]
    L.ndtgpu_mapset_pack_bytes_sparse.restype = C.c_size_t
    L.ndtgpu_mapset_pack_bytes_sparse.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.ndtgpu_mapset_occupied_cells_max.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), vp]
    L.ndtgpu_mapset_pack_cells_sparse_device.argtypes = [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp]
    L.ndtgpu_registrar_create.argtypes = [C.POINTER(GridParams), C.c_size_t, C.c_int, C.POINTER(vp)]
    L.ndtgpu_registrar_destroy.argtypes = [vp]
    L.ndtgpu_default_registrar_params.argtypes = [C.POINTER(RegistrarParams)]
    L.ndtgpu_default_registrar_params.restype = None
    L.ndtgpu_registrar_create_ex.argtypes = [C.POINTER(GridParams), C.POINTER(RegistrarParams), C.POINTER(vp)]
    L.ndtgpu_registrar_get_info.argtypes = [vp, C.POINTER(RegistrarInfo)]
    L.ndtgpu_registrar_inject_abort.argtypes = [vp]
    L.ndtgpu_default_fuser_params.argtypes = [C.POINTER(FuserParams)]
    L.ndtgpu_default_fuser_params.restype = None
    L.ndtgpu_fuser_prepare.argtypes = [C.POINTER(FuserParams), dp, dp, dp, C.POINTER(FuserPrepared)]
    L.ndtgpu_fuser_bank_create.argtypes = [C.POINTER(FuserParams), C.c_size_t, vp, C.POINTER(vp)]
    L.ndtgpu_fuser_bank_destroy.argtypes = [vp]
    L.ndtgpu_fuser_bank_mapsets.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.ndtgpu_fuser_initialize_batch.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp]
    L.ndtgpu_fuser_update_batch.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, vp]
    L.ndtgpu_fuser_poses.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp]
    L.ndtgpu_register_batch_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(CellParams),
                                               vp, C.c_size_t, C.POINTER(MatchParams), vp, vp, C.POINTER(C.c_uint64)]
    L.ndtgpu_register_batch_host.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(CellParams),
                                             dp, C.c_size_t, C.POINTER(MatchParams), vp]
    L.ndtgpu_register_batch_cov_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(CellParams),
                                                   vp, C.c_size_t, C.POINTER(MatchParams), vp, C.c_int, vp, vp, vp, C.POINTER(C.c_uint64)]
    L.ndtgpu_register_batch_cov_host.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(CellParams),
                                                 dp, C.c_size_t, C.POINTER(MatchParams), vp, C.c_int, dp, i32p]
    L.ndtgpu_registrar_wait_stream.argtypes = [vp, C.c_uint64, vp]
    L.ndtgpu_registrar_sync.argtypes = [vp]
    L.ndtgpu_registrar_profiling.argtypes = [vp, C.c_int]
    L.ndtgpu_registrar_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), i32p]
    L.ndtgpu_registrar_mapset.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.ndtgpu_default_resolutions.restype = None
    L.ndtgpu_default_resolutions.argtypes = [dp, i32p]
    L.ndtgpu_multires_create.argtypes = [C.POINTER(GridParams), dp, C.c_int, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_multires_destroy.argtypes = [vp]
    L.ndtgpu_multires_get_info.argtypes = [vp, C.POINTER(MultiResInfo)]
    L.ndtgpu_register_multires_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(CellParams),
                                                  vp, C.c_size_t, C.POINTER(MatchParams), C.c_int, vp, vp]
    L.ndtgpu_register_multires_host.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(CellParams),
                                                dp, C.c_size_t, C.POINTER(MatchParams), C.c_int, vp]
    L.ndtgpu_default_mcl_params.restype = None
    L.ndtgpu_default_mcl_params.argtypes = [C.POINTER(MclParams)]
    L.ndtgpu_mcl_create.argtypes = [vp, u32p, C.POINTER(MclParams), C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_mcl_destroy.argtypes = [vp]
    L.ndtgpu_mcl_initialize.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp]
    L.ndtgpu_mcl_set_particles.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp]
    L.ndtgpu_mcl_update.argtypes = [vp, C.c_size_t, C.c_size_t, dp, C.c_double, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp]
    L.ndtgpu_mcl_update_host.argtypes = [vp, C.c_size_t, C.c_size_t, dp, C.c_double, vp, C.c_size_t, C.c_size_t, C.c_size_t]
    L.ndtgpu_mcl_particles.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp, dp]
    L.ndtgpu_mcl_mean.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp]
    L.ndtgpu_default_pgo_params.restype = None
    L.ndtgpu_default_pgo_params.argtypes = [C.POINTER(PgoParams)]
    L.ndtgpu_pgo_create.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_pgo_destroy.argtypes = [vp]
    L.ndtgpu_pgo_set_graph.argtypes = [vp, C.c_size_t, C.c_size_t, dp, C.c_size_t, u32p, u32p, dp, dp]
    L.ndtgpu_pgo_set_links_device.argtypes = [vp, C.c_size_t, C.c_size_t, dp, C.c_size_t, u32p, u32p, vp, vp, vp]
    L.ndtgpu_pgo_optimize.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(PgoParams), vp]
    L.ndtgpu_pgo_poses.argtypes = [vp, C.c_size_t, dp, dp, C.POINTER(PgoResult)]
    L.ndtgpu_default_pgo_wide_params.restype = None
    L.ndtgpu_default_pgo_wide_params.argtypes = [C.POINTER(PgoWideParams)]
    L.ndtgpu_pgo_wide_plan.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                       C.POINTER(C.c_size_t)]
    L.ndtgpu_pgo_optimize_wide.argtypes = [vp, C.c_size_t, C.POINTER(PgoParams), C.POINTER(PgoWideParams), vp]
    L.ndtgpu_default_pgo3_params.restype = None
    L.ndtgpu_default_pgo3_params.argtypes = [C.POINTER(Pgo3Params)]
    L.ndtgpu_pgo3_create.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_pgo3_destroy.argtypes = [vp]
    L.ndtgpu_pgo3_set_graph.argtypes = [vp, C.c_size_t, C.c_size_t, dp, C.c_size_t, u32p, u32p, dp, dp]
    L.ndtgpu_pgo3_set_links_device.argtypes = [vp, C.c_size_t, C.c_size_t, dp, C.c_size_t, u32p, u32p, vp, vp, vp]
    L.ndtgpu_pgo3_optimize.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(Pgo3Params), vp]
    L.ndtgpu_pgo3_poses.argtypes = [vp, C.c_size_t, dp, C.POINTER(PgoResult)]
    L.ndtgpu_pgo3_link_error.argtypes = [dp, dp, dp, dp, dp, dp]
    L.ndtgpu_pgo3_retract.argtypes = [dp, dp, dp]
    L.ndtgpu_pgo3_link_from_registration.argtypes = [dp, dp, C.c_int32, dp, dp]
    L.ndtgpu_pgo3_wide_plan.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_size_t)]
    L.ndtgpu_pgo3_optimize_wide.argtypes = [vp, C.c_size_t, C.POINTER(Pgo3Params), C.POINTER(PgoWideParams), vp]
    L.ndtgpu_default_pgo_marginal_params.restype = None
    L.ndtgpu_default_pgo_marginal_params.argtypes = [C.POINTER(PgoMarginalParams)]
    L.ndtgpu_pgo_marginal_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int32, C.c_uint64, C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ndtgpu_pgo_marginals.argtypes = [vp, C.c_size_t, u32p, u32p, u32p, C.POINTER(PgoParams), C.POINTER(PgoMarginalParams), dp, dp,
                                       C.POINTER(PgoMarginalResult)]
    L.ndtgpu_pgo_marginals_device.argtypes = [vp, C.c_size_t, u32p, u32p, u32p, C.POINTER(PgoParams), C.POINTER(PgoMarginalParams), vp, vp, vp, vp]
    L.ndtgpu_pgo3_marginals.argtypes = [vp, C.c_size_t, u32p, u32p, u32p, C.POINTER(Pgo3Params), C.POINTER(PgoMarginalParams), dp, dp,
                                        C.POINTER(PgoMarginalResult)]
    L.ndtgpu_pgo3_marginals_device.argtypes = [vp, C.c_size_t, u32p, u32p, u32p, C.POINTER(Pgo3Params), C.POINTER(PgoMarginalParams), vp, vp, vp, vp]
    L.ndtgpu_pgo_relative_covariance.argtypes = [dp, dp, dp, dp, dp, dp]
    L.ndtgpu_pgo3_relative_covariance.argtypes = [dp, dp, dp, dp, dp, dp]
    L.ndtgpu_default_pgo_robust_params.restype = None
    L.ndtgpu_default_pgo_robust_params.argtypes = [C.POINTER(PgoRobustParams)]
    L.ndtgpu_pgo_robust_weight.argtypes = [C.c_int32, C.c_double, C.c_double, dp]
    L.ndtgpu_pgo_optimize_robust.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(PgoParams), C.POINTER(PgoRobustParams),
                                             C.POINTER(PgoWideParams), vp]
    L.ndtgpu_pgo3_optimize_robust.argtypes = [vp, C.c_size_t, C.c_size_t, C.POINTER(Pgo3Params), C.POINTER(PgoRobustParams),
                                              C.POINTER(PgoWideParams), vp]
    for fn in (L.ndtgpu_pgo_robust_links, L.ndtgpu_pgo3_robust_links):
        fn.argtypes = [vp, C.c_size_t, dp, dp, i32p, C.POINTER(PgoRobustResult)]
    for fn in (L.ndtgpu_pgo_robust_links_device, L.ndtgpu_pgo3_robust_links_device):
        fn.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.ndtgpu_pgo_robust_restore.argtypes = [vp, C.c_size_t]
    L.ndtgpu_pgo_link_information.argtypes = [vp, C.c_size_t, dp]
    L.ndtgpu_pgo3_link_information.argtypes = [vp, C.c_size_t, dp]
    L.ndtgpu_pgo3_robust_restore.argtypes = [vp, C.c_size_t]
    L.ndtgpu_default_featmatch_params.restype = None
    L.ndtgpu_default_featmatch_params.argtypes = [C.POINTER(FeatMatchParams)]
    L.ndtgpu_featbank_create.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_featbank_destroy.argtypes = [vp]
    L.ndtgpu_featbank_set.argtypes = [vp, C.c_size_t, C.c_size_t, dp, dp]
    L.ndtgpu_featbank_match.argtypes = [vp, u32p, u32p, C.c_size_t, C.POINTER(FeatMatchParams), vp]
    L.ndtgpu_featbank_match_device.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(FeatMatchParams), vp, vp, vp, vp]
    L.ndtgpu_featbank_results.argtypes = [vp, C.c_size_t, C.c_size_t, vp, dp, u32p]
    L.ndtgpu_default_featextract_params.restype = None
    L.ndtgpu_default_featextract_params.argtypes = [C.POINTER(FeatExtractParams)]
    L.ndtgpu_featbank_extract.argtypes = [vp, u32p, dp, C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.POINTER(FeatExtractParams), vp]
    L.ndtgpu_featbank_extract_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.POINTER(FeatExtractParams),
                                                 vp, vp, vp, vp, vp]
    L.ndtgpu_featbank_extract_results.argtypes = [vp, C.c_size_t, C.c_size_t, vp, u32p, C.POINTER(C.c_int32), dp]
    L.ndtgpu_featbank_get.argtypes = [vp, C.c_size_t, C.POINTER(C.c_size_t), dp, dp]
    L.ndtgpu_default_world_params.restype = None
    L.ndtgpu_default_world_params.argtypes = [C.POINTER(WorldParams)]
    L.ndtgpu_world_assemble.argtypes = [vp, C.c_size_t, C.c_size_t, vp, u32p, u32p, dp, C.POINTER(WorldParams), C.POINTER(WorldResult), vp]
    L.ndtgpu_world_check.argtypes = [C.c_size_t, C.c_double, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, u32p, u32p]
    L.ndtgpu_default_occgrid_params.restype = None
    L.ndtgpu_default_occgrid_params.argtypes = [C.POINTER(OccGridParams)]
    L.ndtgpu_occgrid_dims.argtypes = [C.c_double, C.POINTER(C.c_int32), dp, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32), dp]
    L.ndtgpu_mapset_occupancy_grid_device.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(OccGridParams), vp, vp]
    L.ndtgpu_mapset_occupancy_grid.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(OccGridParams), vp,
                                               C.POINTER(OccGridInfo), vp]
    L.ndtgpu_occgrid_check.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_int32, C.c_int32]
    L.ndtgpu_occgrid_move.restype = None
    L.ndtgpu_occgrid_move.argtypes = [dp, dp, dp]
    L.ndtgpu_default_linkgate_params.restype = None
    L.ndtgpu_default_linkgate_params.argtypes = [C.POINTER(LinkGateParams)]
    L.ndtgpu_linkgate_check.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]
    L.ndtgpu_linkgate_create.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_linkgate_destroy.argtypes = [vp]
    L.ndtgpu_linkgate_set_nodes.argtypes = [vp, C.c_size_t, dp]
    L.ndtgpu_linkgate_set_nodes_device.argtypes = [vp, C.c_size_t, vp, vp]
    L.ndtgpu_linkgate_candidates.argtypes = [vp, C.POINTER(LinkGateParams), vp, vp, vp, C.c_size_t, vp]
    L.ndtgpu_linkgate_valid.argtypes = [vp, C.POINTER(LinkGateParams), C.c_size_t, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.ndtgpu_linkgate_gather.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp]
    L.ndtgpu_linkgate_candidates_host.argtypes = [vp, C.POINTER(LinkGateParams), u32p, u32p, dp, C.c_size_t]
    L.ndtgpu_linkgate_valid_host.argtypes = [vp, C.POINTER(LinkGateParams), C.c_size_t, u32p, u32p, dp, dp]
    L.ndtgpu_linkgate_count.argtypes = [vp, C.POINTER(C.c_size_t), i32p]
    L.ndtgpu_linkgate_keep.argtypes = [vp, C.c_size_t, C.c_size_t, u32p]
    L.ndtgpu_default_fuser_feat_params.restype = None
    L.ndtgpu_default_fuser_feat_params.argtypes = [C.POINTER(FuserFeatParams)]
    L.ndtgpu_fuser_feat_prepare.argtypes = [C.POINTER(FuserParams), C.POINTER(FuserFeatParams), dp, dp, C.POINTER(FeatMatchResult), u32p, dp,
                                            C.c_size_t, dp, C.c_size_t, C.c_int, C.POINTER(FuserFeatResult), dp, u32p]
    L.ndtgpu_fuser_feat_move.argtypes = [dp, dp, C.c_size_t, dp]
    L.ndtgpu_fuser_bank_attach_features.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(FuserFeatParams)]
    L.ndtgpu_fuser_initialize_batch_feat.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp, C.c_size_t, C.c_size_t, C.c_size_t, u32p, vp]
    L.ndtgpu_fuser_update_batch_feat.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp, C.c_size_t, C.c_size_t, C.c_size_t, u32p, C.c_int, C.c_int, vp]
    L.ndtgpu_fuser_initialize_batch_feat_host.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp, C.c_size_t, C.c_size_t, C.c_size_t, u32p]
    L.ndtgpu_fuser_update_batch_feat_host.argtypes = [vp, C.c_size_t, C.c_size_t, dp, vp, C.c_size_t, C.c_size_t, C.c_size_t, u32p, C.c_int,
                                                      C.c_int]
    L.ndtgpu_fuser_feat_results.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
    L.ndtgpu_fuser_feat_cells.argtypes = [vp, C.c_size_t, C.c_size_t, u32p, dp, C.c_size_t]
    L.ndtgpu_default_scanproject_params.restype = None
    L.ndtgpu_default_scanproject_params.argtypes = [C.POINTER(ScanProjectParams)]
    L.ndtgpu_scanproj_tile.restype = C.c_uint32
    L.ndtgpu_scanproj_tile.argtypes = []
    L.ndtgpu_scanproj_check.argtypes = [C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.c_size_t, C.c_size_t, C.POINTER(ScanProjectParams)]
    L.ndtgpu_scanproj_beam.argtypes = [C.POINTER(ScanProjectParams), C.c_double, C.c_double, C.c_uint64, C.c_uint32, C.c_double,
                                       C.POINTER(C.c_float)]
    L.ndtgpu_scanproj_create.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_scanproj_destroy.argtypes = [vp]
    L.ndtgpu_scanproj_project_device.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.POINTER(ScanProjectParams),
                                                 vp, C.c_size_t, C.c_size_t, vp, vp]
    L.ndtgpu_scanproj_project.argtypes = [vp, dp, C.POINTER(C.c_uint64), C.c_size_t, C.c_size_t, C.c_double, C.c_double,
                                          C.POINTER(ScanProjectParams), vp, C.c_size_t, C.c_size_t, u32p]
    L.ndtgpu_default_calib_params.restype = None
    L.ndtgpu_default_calib_params.argtypes = [C.POINTER(CalibParams)]
    L.ndtgpu_calib_tile.restype = C.c_uint32
    L.ndtgpu_calib_tile.argtypes = []
    L.ndtgpu_calib_lattice.argtypes = [C.c_double] * 8 + [C.POINTER(C.c_size_t), dp, dp, dp, dp, dp, C.c_size_t]
    L.ndtgpu_calib_pair_motion.argtypes = [dp, dp, dp]
    L.ndtgpu_calib_select_pairs.argtypes = [dp, C.c_size_t, C.c_double, C.c_double, u32p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ndtgpu_calib_check.argtypes = [C.c_size_t] * 8 + [C.POINTER(CalibParams)]
    L.ndtgpu_calib_create.argtypes = [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.ndtgpu_calib_destroy.argtypes = [vp]
    L.ndtgpu_calib_search_device.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, vp, C.c_size_t, dp, C.c_size_t, dp,
                                             C.c_size_t, dp, dp, C.c_size_t, C.POINTER(CalibParams), vp, vp, vp]
    L.ndtgpu_calib_search.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, u32p, dp, u32p, C.c_size_t, dp, C.c_size_t, dp,
                                      C.c_size_t, dp, dp, C.c_size_t, C.POINTER(CalibParams), C.POINTER(CalibResult), dp]
    sz, i32, u32 = C.c_size_t, C.c_int32, C.c_uint32
    lp = C.POINTER(LocmonParams)
    L.ndtgpu_default_locmon_params.restype = None
    L.ndtgpu_default_locmon_params.argtypes = [lp]
    L.ndtgpu_locmon_tile.restype = u32
    L.ndtgpu_locmon_tile.argtypes = []
    L.ndtgpu_locmon_check.argtypes = [sz, sz, sz, C.c_double, sz, C.c_double, C.c_double, sz, sz, lp]
    L.ndtgpu_locmon_radius.argtypes = [C.c_double, C.c_double, i32p]
    L.ndtgpu_locmon_beam_table.argtypes = [sz, C.c_double, C.c_double, dp, dp]
    L.ndtgpu_locmon_pixel.argtypes = [dp, C.c_double, C.c_double, C.c_double, dp, C.c_double, u32, u32, i32p, i32p]
    L.ndtgpu_locmon_metres.argtypes = [u32, C.c_double, C.c_double, dp]
    L.ndtgpu_locmon_compose.argtypes = [dp, dp, dp, dp]
    L.ndtgpu_locmon_create.argtypes = [sz, sz, sz, sz, C.POINTER(vp)]
    L.ndtgpu_locmon_destroy.argtypes = [vp]
    L.ndtgpu_locmon_set_beams.argtypes = [vp, sz, C.c_double, C.c_double, vp]
    L.ndtgpu_locmon_set_grids_device.argtypes = [vp, vp, sz, sz, sz, C.c_double, dp, lp, vp]
    L.ndtgpu_locmon_set_grids.argtypes = [vp, vp, sz, sz, sz, C.c_double, dp, lp]
    L.ndtgpu_locmon_field_get.argtypes = [vp, sz, vp]
    L.ndtgpu_locmon_evaluate_device.argtypes = [vp, vp, sz, vp, sz, lp, vp, vp]
    L.ndtgpu_locmon_evaluate.argtypes = [vp, dp, sz, vp, sz, lp, vp]
    L.ndtgpu_locmon_adjust_device.argtypes = [vp, vp, sz, u32, u32, dp, sz, dp, sz, dp, dp, sz, lp, vp, vp, vp]
    L.ndtgpu_locmon_adjust.argtypes = [vp, dp, sz, u32, u32, dp, sz, dp, sz, dp, dp, sz, lp, C.POINTER(LocmonAdjustResult), u32p]
    L.ndtgpu_locmon_pick_device.argtypes = [vp, vp, vp, sz, u32, u32, lp, vp, vp, vp]
    ssp = C.POINTER(ScansimParams)
    L.ndtgpu_default_scansim_params.restype = None
    L.ndtgpu_default_scansim_params.argtypes = [ssp]
    L.ndtgpu_scansim_tile.restype = u32
    L.ndtgpu_scansim_tile.argtypes = []
    L.ndtgpu_scansim_check.argtypes = [sz, sz, sz, C.c_double, sz, C.c_double, C.c_double, sz, ssp]
    L.ndtgpu_scansim_reach.argtypes = [C.c_double, C.c_double, i32p]
    L.ndtgpu_scansim_skip.argtypes = [C.c_double, C.c_double, u32p]
    L.ndtgpu_scansim_cell.argtypes = [C.c_int32, C.c_int32, C.c_int32, i32p]
    L.ndtgpu_scansim_beam.argtypes = [vp, sz, sz, dp, C.c_double, dp, C.c_double, C.c_double, ssp, dp, i32p, u32p]
    L.ndtgpu_scansim_headings.argtypes = [C.c_double, C.POINTER(sz), dp, dp, sz]
    L.ndtgpu_scansim_create.argtypes = [sz, sz, sz, C.POINTER(vp)]
    L.ndtgpu_scansim_destroy.argtypes = [vp]
    L.ndtgpu_scansim_set_beams.argtypes = [vp, sz, C.c_double, C.c_double, vp]
    L.ndtgpu_scansim_set_grids_device.argtypes = [vp, vp, sz, sz, sz, C.c_double, dp, vp]
    L.ndtgpu_scansim_set_grids.argtypes = [vp, vp, sz, sz, sz, C.c_double, dp]
    L.ndtgpu_scansim_lattice_device.argtypes = [vp, u32, u32, dp, dp, sz, dp, sz, vp, vp, vp, vp]
    L.ndtgpu_scansim_lattice.argtypes = [vp, u32, u32, dp, dp, sz, dp, sz, dp, u32p, u32p]
    L.ndtgpu_scansim_simulate_device.argtypes = [vp, vp, vp, sz, vp, ssp, vp, vp, vp]
    L.ndtgpu_scansim_simulate.argtypes = [vp, dp, u32p, sz, ssp, dp, vp]
    mkp = C.POINTER(MarkerParams)
    L.ndtgpu_default_marker_params.restype = None
    L.ndtgpu_default_marker_params.argtypes = [mkp]
    L.ndtgpu_marker_tile.restype = u32
    L.ndtgpu_marker_tile.argtypes = []
    L.ndtgpu_marker_check.argtypes = [sz, sz, sz, sz, sz, sz, sz, sz, sz, mkp]
    L.ndtgpu_marker_eig3.argtypes = [dp, dp, dp]
    L.ndtgpu_marker_cell.argtypes = [dp, dp, dp, mkp, dp, dp, u32p, u32p]
    L.ndtgpu_marker_create.argtypes = [sz, sz, C.POINTER(vp)]
    L.ndtgpu_marker_destroy.argtypes = [vp]
    L.ndtgpu_mapset_markers_device.argtypes = [vp, vp, sz, sz, vp, mkp, vp, vp, sz, vp]
    L.ndtgpu_mapset_markers.argtypes = [vp, vp, sz, sz, dp, mkp, dp, u32p, sz, C.POINTER(sz), i32p, u32p]
    L.ndtgpu_marker_count.argtypes = [vp, C.POINTER(sz), i32p, u32p]
    L.ndtgpu_marker_links_device.argtypes = [vp, vp, sz, vp, vp, vp, sz, mkp, vp, sz, vp]
    L.ndtgpu_marker_links.argtypes = [vp, dp, sz, u32p, u32p, dp, sz, mkp, dp, sz, C.POINTER(sz), i32p]
    L.ndtgpu_mcl_markers_device.argtypes = [vp, sz, sz, mkp, vp, vp]
    L.ndtgpu_mcl_markers.argtypes = [vp, sz, sz, mkp, dp]
    if hasattr(L, "ndtgpu_live_resources"):            # (NDTGPU_LIB may name a build from before this entry existed)
        L.ndtgpu_live_resources.argtypes = [C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise NdtGpuError(rc, lib().ndtgpu_last_error().decode())


def device_count():
    return lib().ndtgpu_device_count()


def live_resources():
    """test aid (ndtgpu_live_resources): what the library owns right now, process-wide -- (device buffers, pinned buffers, events, streams)"""
    c = (C.c_uint64 * 4)()
    _check(lib().ndtgpu_live_resources(c))
    return tuple(int(x) for x in c)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _params(struct_type, default_fn, label, fields, hidden=()):
    """the library's defaults (default_fn names the ndtgpu_default_* function) with `fields` replaced; a field that is an array takes
    a sequence of numbers"""
    p = struct_type()
    getattr(lib(), default_fn)(C.byref(p))
    for k, v in fields.items():
        if not hasattr(p, k) or k in hidden:
            raise TypeError("unknown %s parameter %r" % (label, k))
        if isinstance(getattr(p, k), C.Array):
            getattr(p, k)[:] = [float(x) for x in np.asarray(v, dtype=np.float64).ravel()]
        else:
            setattr(p, k, v)
    return p


class _Handle:
    """close / __del__ of a class that keeps a handle of the library in self.h; _destroy names the function that destroys it"""
    _destroy = None

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_params(**kw):
    return _params(MatchParams, "ndtgpu_default_match_params", "match", kw)


def _stream_ptr(stream):
    if stream is None:
        return None
    if hasattr(stream, "cuda_stream"):
        return C.c_void_p(stream.cuda_stream)
    return C.c_void_p(int(stream))


class MapSet(_Handle):
    """B x lslgeneric::NDTMap(new LazyGrid(res)) with one grid geometry, resident in HBM."""
    _destroy = "ndtgpu_mapset_destroy"

    def __init__(self, res, centre, size_m, n_maps=1, max_cells=0):
        L = lib()
        gp = GridParams()
        gp.res = float(res)
        gp.centre[:] = [float(x) for x in centre]
        gp.size[:] = [float(x) for x in size_m]
        gp.max_cells = int(max_cells)
        h = C.c_void_p()
        _check(L.ndtgpu_mapset_create(C.byref(gp), int(n_maps), C.byref(h)))
        self.h = h
        self.n_maps = int(n_maps)
        self.res = float(res)

    def info(self):
        n = C.c_size_t()
        cells = (C.c_int32 * 3)()
        cap = C.c_uint32()
        _check(lib().ndtgpu_mapset_info(self.h, C.byref(n), cells, C.byref(cap)))
        return dict(n_maps=n.value, cells_per_axis=list(cells), max_cells=cap.value)

    def set_centre(self, i, centre):
        c = _f64(centre)
        _check(lib().ndtgpu_mapset_set_centre(self.h, int(i), _dp(c)))

    def build(self, xyz, range_limit=-1.0, range_origins=None, first=0, n_min=3, eval_factor=1000.0, stream=None):
        """loadPointCloud + computeNDTCells for maps [first, first+B).  xyz: [B,N,3|4] float32,
        a torch CUDA tensor (device path, asynchronous) or a NumPy array (host path)."""
        cp = CellParams(int(n_min), float(eval_factor))
        ro = None
        is_torch = hasattr(xyz, "data_ptr")
        if xyz.ndim == 2:
            xyz = xyz[None]
        B, N, W = int(xyz.shape[0]), int(xyz.shape[1]), int(xyz.shape[2])
        assert W in (3, 4)
        if range_origins is not None:
            ro = _f64(range_origins).reshape(B, 3)
        rop = _dp(ro) if ro is not None else None
        if is_torch:
            import torch
            assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous()
            if stream is None:
                stream = torch.cuda.current_stream()
            _check(lib().ndtgpu_mapset_build(self.h, int(first), B, C.c_void_p(xyz.data_ptr()), N, 4 * W, 4 * W * N,
                                             float(range_limit), rop, C.byref(cp), _stream_ptr(stream)))
        else:
            a = np.ascontiguousarray(xyz, dtype=np.float32)
            if stream is not None:      # asynchronous host form: returns when `a` has been read, the maps are ready when `stream` is
                _check(lib().ndtgpu_mapset_build_host_async(self.h, int(first), B, C.c_void_p(a.ctypes.data), N, 4 * W,
                                                            4 * W * N, float(range_limit), rop, C.byref(cp), _stream_ptr(stream)))
            else:
                _check(lib().ndtgpu_mapset_build_host(self.h, int(first), B, C.c_void_p(a.ctypes.data), N, 4 * W,
                                                      4 * W * N, float(range_limit), rop, C.byref(cp)))

    def enable_occupancy(self):
        """NDTMap::initialize: every cell exists and carries an occupancy; needed by add_cloud / overlap_score."""
        _check(lib().ndtgpu_mapset_enable_occupancy(self.h))

    def add_cloud(self, xyz, origins, first=0, stream=None, **params):
        """NDTMap::addPointCloud(origin, cloud, ., maxz, sensor_noise) + computeNDTCells(SAMPLE_VARIANCE, maxnumpoints,
        occupancy_limit, ..) for maps [first, first+B): xyz [B,N,3|4] float32 (torch CUDA tensor: asynchronous; NumPy:
        host path), origins [B,3] sensor positions in the map frame."""
        fp = FuseParams()
        lib().ndtgpu_default_fuse_params(C.byref(fp))
        for k, v in params.items():
            if not hasattr(fp, k):
                raise TypeError("unknown fuse parameter %r" % k)
            setattr(fp, k, v)
        is_torch = hasattr(xyz, "data_ptr")
        if xyz.ndim == 2:
            xyz = xyz[None]
        B, N, W = int(xyz.shape[0]), int(xyz.shape[1]), int(xyz.shape[2])
        assert W in (3, 4)
        org = _f64(origins).reshape(B, 3)
        if is_torch:
            import torch
            assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous()
            if stream is None:
                stream = torch.cuda.current_stream()
            _check(lib().ndtgpu_mapset_add_cloud(self.h, int(first), B, C.c_void_p(xyz.data_ptr()), N, 4 * W, 4 * W * N,
                                                 _dp(org), C.byref(fp), _stream_ptr(stream)))
        else:
            a = np.ascontiguousarray(xyz, dtype=np.float32)
            _check(lib().ndtgpu_mapset_add_cloud_host(self.h, int(first), B, C.c_void_p(a.ctypes.data), N, 4 * W, 4 * W * N,
                                                      _dp(org), C.byref(fp)))

    def discard_cells(self, i, xyz):
        """ndt_feature::discardCell for every point: the cells that hold them lose their Gaussian."""
        a = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        _check(lib().ndtgpu_mapset_discard_cells(self.h, int(i), a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0]))

    def clear(self, first=0, count=None):
        _check(lib().ndtgpu_mapset_clear(self.h, int(first), int(self.n_maps - first if count is None else count)))

    def occupancy(self, i=0):
        """NDTCell::occ of every cell of map i, shape (sx, sy, sz)."""
        shape = tuple(self.info()["cells_per_axis"])
        out = np.zeros(shape, dtype=np.float32)
        _check(lib().ndtgpu_mapset_export_occupancy(self.h, int(i), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def pack_bytes(self, cells_cap, with_occupancy=False, occ_cap=None):
        """Bytes of one exchange record.  occ_cap: the sparse form of the occupancy block (room for that many cells with a
        reading, ndtgpu_mapset_pack_bytes_sparse) instead of one float per slot."""
        if occ_cap is not None:
            return int(lib().ndtgpu_mapset_pack_bytes_sparse(self.h, int(cells_cap), int(occ_cap)))
        return int(lib().ndtgpu_mapset_pack_bytes(self.h, int(cells_cap), int(bool(with_occupancy))))

    def occupied_cells_max(self, first=0, count=None, stream=None):
        """The largest number of cells with an occupancy reading over maps [first, first+count): what the occ_cap of a
        sparse exchange record must hold (ndtgpu_mapset_occupied_cells_max; synchronises the stream)."""
        import torch
        count = self.n_maps - first if count is None else count
        if stream is None:
            stream = torch.cuda.current_stream()
        out = C.c_uint32()
        _check(lib().ndtgpu_mapset_occupied_cells_max(self.h, int(first), int(count), C.byref(out), _stream_ptr(stream)))
        return int(out.value)

    def pack_cells(self, buf, first=0, count=None, cells_cap=None, with_occupancy=False, stream=None, occ_cap=None):
        """Exchange records of maps [first, first+count) into the torch CUDA uint8 tensor buf [count, stride]
        (ndtgpu_mapset_pack_cells_device; asynchronous).  occ_cap: occupancies as (slot, value) pairs of the cells with a
        reading (ndtgpu_mapset_pack_cells_sparse_device)."""
        import torch
        count = self.n_maps - first if count is None else count
        cap = self.info()["max_cells"] if cells_cap is None else cells_cap
        assert buf.dtype == torch.uint8 and buf.is_cuda and buf.is_contiguous() and buf.shape[0] >= count
        if stream is None:
            stream = torch.cuda.current_stream()
        if occ_cap is not None:
            _check(lib().ndtgpu_mapset_pack_cells_sparse_device(self.h, int(first), int(count), C.c_void_p(buf.data_ptr()),
                                                                int(buf.stride(0)), int(cap), int(occ_cap), _stream_ptr(stream)))
            return
        _check(lib().ndtgpu_mapset_pack_cells_device(self.h, int(first), int(count), C.c_void_p(buf.data_ptr()), int(buf.stride(0)),
                                                     int(cap), int(bool(with_occupancy)), _stream_ptr(stream)))

    def unpack_cells(self, buf, first=0, count=None, with_occupancy=False, stream=None):
        """Installs exchange records (ndtgpu_mapset_unpack_cells_device; asynchronous)."""
        import torch
        count = buf.shape[0] if count is None else count
        assert buf.dtype == torch.uint8 and buf.is_cuda and buf.is_contiguous()
        if stream is None:
            stream = torch.cuda.current_stream()
        _check(lib().ndtgpu_mapset_unpack_cells_device(self.h, int(first), int(count), C.c_void_p(buf.data_ptr()), int(buf.stride(0)),
                                                       int(bool(with_occupancy)), _stream_ptr(stream)))

    def profiling(self, on=True):
        _check(lib().ndtgpu_profiling_enable(self.h, int(bool(on))))

    def last_kernel_ms(self, which):
        """HIP-event duration of the most recent build (0) / match (1) kernel launched on this set."""
        ms = C.c_float()
        _check(lib().ndtgpu_last_kernel_ms(self.h, int(which), C.byref(ms)))
        return ms.value

    def counters(self, i=0):
        out = (C.c_uint32 * 8)()
        _check(lib().ndtgpu_mapset_counters(self.h, int(i), out))
        return dict(n_alloc=out[0], n_cells=out[1], overflow=out[2], n_dropped=out[3], cyc=list(out[4:8]))

    def num_cells_all(self):
        """n_cells of every map (one D2H of the counters; synchronises)."""
        return np.array([self.num_cells(i) for i in range(self.n_maps)], dtype=np.int64)

    def num_cells(self, i=0):
        n = C.c_uint32()
        _check(lib().ndtgpu_mapset_num_cells(self.h, int(i), C.byref(n)))
        return n.value

    def export_cells(self, i=0):
        n = self.num_cells(i)
        mean = np.zeros((n, 3))
        cov = np.zeros((n, 3, 3))
        idx = np.zeros((n, 3), dtype=np.int32)
        npts = np.zeros(n, dtype=np.uint32)
        _check(lib().ndtgpu_mapset_export_cells(self.h, int(i), _dp(mean), _dp(cov),
                                                idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                npts.ctypes.data_as(C.POINTER(C.c_uint32))))
        return mean, cov, idx, npts

    def set_cells(self, i, mean, cov):
        mean, cov = _f64(mean).reshape(-1, 3), _f64(cov).reshape(-1, 3, 3)
        _check(lib().ndtgpu_mapset_set_cells(self.h, int(i), _dp(mean), _dp(cov), mean.shape[0]))

    def occupancy_grid(self, first, count, resolution, z=0.0, occupied_no_gaussian=100, out=None, stream=None):
        """lslgeneric::toOccupancyGrid of maps [first, first + count) at pixel size `resolution` (ndtgpu_mapset_occupancy_grid):
        returns (int8 array [count, height, width], info) -- info: one dict per map (width, height, resolution, origin and the
        counts n_unknown / n_free / n_occupied).  out: a torch CUDA int8 tensor of count * height * width elements takes the
        device form (ndtgpu_mapset_occupancy_grid_device, asynchronous on `stream`); it is returned, reshaped, instead of an
        array, and the infos then carry width, height and resolution only (the origin: occupancy_grid_dims with the map's
        centre)."""
        p = occgrid_params(z=float(z), occupied_no_gaussian=int(occupied_no_gaussian))
        first, count = int(first), int(count)
        cpa = self.info()["cells_per_axis"]
        w, h, _ = occupancy_grid_dims(self.res, cpa, [0.0, 0.0, 0.0], resolution)
        _check(lib().ndtgpu_occgrid_check(self.n_maps, first, count, w, h))           # (before anything of that size is allocated)
        infos = [dict(width=w, height=h, resolution=float(resolution)) for _ in range(count)]
        if out is not None:
            import torch
            assert out.dtype == torch.int8 and out.is_cuda and out.is_contiguous() and out.numel() == count * h * w
            if stream is None:
                stream = torch.cuda.current_stream()
            _check(lib().ndtgpu_mapset_occupancy_grid_device(self.h, first, count, float(resolution), C.byref(p), C.c_void_p(out.data_ptr()),
                                                             _stream_ptr(stream)))
            return out.view(count, h, w), infos
        grid = np.empty((count, h, w), dtype=np.int8)
        rec = (OccGridInfo * max(count, 1))()
        buf = grid if grid.size else np.empty(1, dtype=np.int8)          # (never an empty buffer)
        _check(lib().ndtgpu_mapset_occupancy_grid(self.h, first, count, float(resolution), C.byref(p), C.c_void_p(buf.ctypes.data), rec,
                                                  _stream_ptr(stream)))
        for k in range(count):
            infos[k] = dict(width=rec[k].width, height=rec[k].height, resolution=rec[k].resolution, origin=list(rec[k].origin),
                            n_unknown=rec[k].n_unknown, n_free=rec[k].n_free, n_occupied=rec[k].n_occupied)
        return grid, infos

    def markers(self, first, count, poses=None, marker=None, capacity=None, want_src=True, **params):
        """ndt_visualisation::markerNDTCells of maps [first, first + count) (ndtgpu_mapset_markers): the axis segments of every
        Gaussian cell in (map, cell, axis) order, each map under its pose (poses [count, 4, 4] or None) -> (points [n, 2, 3], src
        uint32 [n, 2] = (map, cell rank) or None, info dict(n_segments, overflow, flags)).  capacity None: three segments a cell.
        marker: a Marker to reuse (None: one is made for the call).  Keyword arguments: fields of ndtgpu_marker_params.  Synchronous."""
        first, count = int(first), int(count)
        own = marker is None
        if own:
            marker = Marker(max(count, 1), 0)
        try:
            if capacity is None:
                capacity = 3 * sum(self.num_cells(i) for i in range(first, first + count))
            return marker.cells(self, first, count, poses=poses, capacity=capacity, want_src=want_src, **params)
        finally:
            if own:
                marker.close()

    def markers_device(self, marker, first, count, points_t, src_t=None, poses_t=None, capacity=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream` (ndtgpu_mapset_markers_device): points_t float64 [capacity, 6],
        src_t int32 [capacity, 2] or None (read as uint32), poses_t float64 [count, 16] column-major or None; the counts stay with
        `marker` (Marker.count)"""
        marker.cells_device(self, first, count, points_t, src_t=src_t, poses_t=poses_t, capacity=capacity, stream=stream, **params)


def derivatives(target, tmap, src_mean, src_cov, n_neighbours=2, compute_hessian=True, lfd1=1.0, lfd2=0.05):
    """NDTMatcherD2D::derivativesNDT on the device (source cells already in the target frame)."""
    src_mean, src_cov = _f64(src_mean).reshape(-1, 3), _f64(src_cov).reshape(-1, 3, 3)
    s = C.c_double()
    g = np.zeros(6)
    H = np.zeros((6, 6))
    _check(lib().ndtgpu_derivatives(target.h, int(tmap), _dp(src_mean), _dp(src_cov), src_mean.shape[0],
                                    int(n_neighbours), int(bool(compute_hessian)), lfd1, lfd2, C.byref(s), _dp(g), _dp(H)))
    return s.value, g, H


def match_batch(target_set, target_idx, source_set, source_idx, T, stream=None, **params):
    """NDTFeatureGraph::updateLinksUsingNDTRegistration's loop: match(target, source, T, true) for every
    pair.  T: [n,4,4] (math convention); returns (T_out [n,4,4], results structured array)."""
    ti = np.ascontiguousarray(target_idx, dtype=np.uint32)
    si = np.ascontiguousarray(source_idx, dtype=np.uint32)
    n = ti.shape[0]
    Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
    res = np.zeros(n, dtype=RESULT_DTYPE)
    p = match_params(**params)
    _check(lib().ndtgpu_match_batch(target_set.h, ti.ctypes.data_as(C.POINTER(C.c_uint32)), source_set.h,
                                    si.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(Tc), n, C.byref(p),
                                    C.c_void_p(res.ctypes.data), _stream_ptr(stream)))
    return np.transpose(Tc, (0, 2, 1)).copy(), res


def match_fusion_batch(target_set, target_idx, source_set, source_idx, T, Tcov, use_soft_constraints=True, stream=None,
                       tikhonov=False, **params):
    """ndt_feature::matchFusion (NDT term + odometry soft constraint and / or Tikhonov regularisation) for every pair.
    Tcov: [n,6,6]."""
    ti = np.ascontiguousarray(target_idx, dtype=np.uint32)
    si = np.ascontiguousarray(source_idx, dtype=np.uint32)
    n = ti.shape[0]
    Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
    cov = np.ascontiguousarray(np.asarray(Tcov, dtype=np.float64).reshape(n, 36))
    res = np.zeros(n, dtype=RESULT_DTYPE)
    p = match_params(**params)
    _check(lib().ndtgpu_match_fusion_batch(target_set.h, ti.ctypes.data_as(C.POINTER(C.c_uint32)), source_set.h,
                                           si.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(Tc), _dp(cov), n, C.byref(p),
                                           int(bool(use_soft_constraints)) | (2 if tikhonov else 0), C.c_void_p(res.ctypes.data),
                                           _stream_ptr(stream)))
    return np.transpose(Tc, (0, 2, 1)).copy(), res


class FeatPairs(C.Structure):
    _fields_ = [("offsets", C.POINTER(C.c_uint32)), ("src_mean", C.POINTER(C.c_double)), ("src_cov", C.POINTER(C.c_double)),
                ("tgt_mean", C.POINTER(C.c_double)), ("tgt_cov", C.POINTER(C.c_double))]


def match_fusion_feat_batch(target_set, target_idx, source_set, source_idx, T, Tcov, feat, use_soft_constraints=True,
                            tikhonov=False, step_control_fusion=False, stream=None, **params):
    """ndt_feature::matchFusion with feature / odometry-cell maps.  feat: one entry per pair, each a tuple
    (src_mean [k,3], src_cov [k,6], tgt_mean [k,3], tgt_cov [k,6]) of k <= 64 corresponding cells (k may be 0)."""
    ti = np.ascontiguousarray(target_idx, dtype=np.uint32)
    si = np.ascontiguousarray(source_idx, dtype=np.uint32)
    n = ti.shape[0]
    Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
    cov = np.ascontiguousarray(np.asarray(Tcov, dtype=np.float64).reshape(n, 36))
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(f[0]) for f in feat])
    cat = lambda j, w: np.ascontiguousarray(np.concatenate([np.asarray(f[j], dtype=np.float64).reshape(-1, w) for f in feat]
                                                           + [np.zeros((1, w))]))
    sm, sc, tm, tc = cat(0, 3), cat(1, 6), cat(2, 3), cat(3, 6)
    fp = FeatPairs(off.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(sm), _dp(sc), _dp(tm), _dp(tc))
    res = np.zeros(n, dtype=RESULT_DTYPE)
    p = match_params(**params)
    L = lib()
    L.ndtgpu_match_fusion_feat_batch.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(FeatPairs), C.c_size_t,
                                                 C.POINTER(MatchParams), C.c_int, C.c_void_p, C.c_void_p]
    flags = int(bool(use_soft_constraints)) | (2 if tikhonov else 0) | (4 if step_control_fusion else 0)
    _check(L.ndtgpu_match_fusion_feat_batch(target_set.h, ti.ctypes.data_as(C.POINTER(C.c_uint32)), source_set.h,
                                            si.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(Tc), _dp(cov), C.byref(fp), n,
                                            C.byref(p), flags, C.c_void_p(res.ctypes.data), _stream_ptr(stream)))
    return np.transpose(Tc, (0, 2, 1)).copy(), res


def match_aborted(target_set):
    """True when the last persistent matcher launch on this target set gave up (waits for that launch)."""
    a = C.c_int32()
    _check(lib().ndtgpu_match_aborted(target_set.h, C.byref(a)))
    return bool(a.value)


def match_batch_device(target_set, tidx_dev, source_set, sidx_dev, T16_dev, results_dev, n_pairs, stream=None, **params):
    """Asynchronous device-resident variant (torch CUDA tensors: uint32/int32 idx, float64 [n,16]
    column-major poses, uint8 [n,64] results)."""
    p = match_params(**params)
    _check(lib().ndtgpu_match_batch_device(target_set.h, C.c_void_p(tidx_dev.data_ptr()), source_set.h,
                                           C.c_void_p(sidx_dev.data_ptr()), C.c_void_p(T16_dev.data_ptr()), int(n_pairs),
                                           C.byref(p), C.c_void_p(results_dev.data_ptr()), _stream_ptr(stream)))


class _BorrowedMapSet(MapSet):
    """A map set owned by somebody else (a registrar): same methods, never destroyed from here."""

    def __init__(self, h, n_maps, res):
        self.h, self.n_maps, self.res = h, int(n_maps), float(res)

    def close(self):
        self.h = None


class RegistrarParams(C.Structure):
    _fields_ = [("pairs_per_batch", C.c_size_t), ("depth", C.c_int32), ("matcher_form", C.c_int32), ("matcher_groups", C.c_uint32),
                ("build_streams", C.c_int32), ("linger_us", C.c_uint32), ("recalibrate_pct", C.c_int32), ("matcher_slots", C.c_int32)]


class RegistrarInfo(C.Structure):
    _fields_ = [("matcher_form", C.c_int32), ("matcher_groups", C.c_uint32), ("build_streams", C.c_int32), ("calibrations", C.c_int32),
                ("submitted", C.c_uint64), ("cells_per_map", C.c_double), ("matcher_slots", C.c_int32), ("resident_groups", C.c_int32)]


MATCHER_AUTO, MATCHER_PER_BATCH, MATCHER_STREAM_FED = 0, 1, 2
# the registrar's covariance flags (include/ndtgpu.h NDTGPU_COV_*)
COV_SINGULAR, COV_POSE_UNCHANGED, COV_NOT_COMPUTED = 1, 2, 4


class Registrar(_Handle):
    """ndtgpu_registrar: scans in, poses out -- grid builds + D2D matcher of batches of scan pairs as ONE asynchronous call,
    pipelined over the library's own streams (include/ndtgpu.h).  Keyword arguments beyond pairs_per_batch / depth are the
    fields of ndtgpu_registrar_params (matcher_form, matcher_groups, build_streams, linger_us, recalibrate_pct)."""
    _destroy = "ndtgpu_registrar_destroy"

    def __init__(self, res, centre, size_m, pairs_per_batch=1024, depth=8, max_cells=0, **fields):
        gp = GridParams()
        gp.res = float(res)
        gp.centre[:] = [float(x) for x in centre]
        gp.size[:] = [float(x) for x in size_m]
        gp.max_cells = int(max_cells)
        rp = RegistrarParams()
        lib().ndtgpu_default_registrar_params(C.byref(rp))
        rp.pairs_per_batch, rp.depth = int(pairs_per_batch), int(depth)
        for k, v in fields.items():
            if k not in dict(RegistrarParams._fields_):
                raise TypeError("Registrar: no parameter %r" % k)
            setattr(rp, k, int(v))
        h = C.c_void_p()
        _check(lib().ndtgpu_registrar_create_ex(C.byref(gp), C.byref(rp), C.byref(h)))
        self.h, self.depth, self.per, self.res = h, int(depth), int(pairs_per_batch), float(res)

    def inject_abort(self):
        """test aid: the stream-fed matcher's give-up word (include/ndtgpu.h)"""
        _check(lib().ndtgpu_registrar_inject_abort(self.h))

    def info(self):
        i = RegistrarInfo()
        _check(lib().ndtgpu_registrar_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in RegistrarInfo._fields_}

    def submit(self, targets, sources, T16_dev, results_dev, range_limit=-1.0, n_min=3, eval_factor=1000.0, stream=None,
               covariance_mode=None, cov36_dev=None, cov_flags_dev=None, **params):
        """targets / sources: torch CUDA float32 tensors [n, N, 3 or 4] (contiguous in the last two dims); T16_dev float64
        [n, 16] column-major (in: initial guess, out: pose); results_dev uint8 [n, 64].  Asynchronous; returns the call's
        ticket (wait_stream / sync).  covariance_mode 0 / 1 (ndtgpu_register_batch_cov_device): also the covariance of every
        pair at its registered pose into cov36_dev (float64 [n, 36], row-major 6x6) and cov_flags_dev (int32 [n], COV_*)."""
        n, npts = int(targets.shape[0]), int(targets.shape[1])
        assert tuple(sources.shape) == tuple(targets.shape) and targets.stride(1) == targets.shape[2] and targets.stride(2) == 1
        assert sources.stride(0) == targets.stride(0) and sources.stride(1) == targets.stride(1) and sources.stride(2) == 1
        cp = CellParams(int(n_min), float(eval_factor))
        p = match_params(**params)
        t = C.c_uint64()
        args = (self.h, C.c_void_p(targets.data_ptr()), C.c_void_p(sources.data_ptr()), npts, 4 * int(targets.shape[2]),
                4 * int(targets.stride(0)), float(range_limit), C.byref(cp), C.c_void_p(T16_dev.data_ptr()), n, C.byref(p),
                C.c_void_p(results_dev.data_ptr()))
        if covariance_mode is None:
            _check(lib().ndtgpu_register_batch_device(*args, _stream_ptr(stream), C.byref(t)))
        else:
            for a, what in ((cov36_dev, "cov36_dev"), (cov_flags_dev, "cov_flags_dev")):
                if a is None:
                    raise ValueError("Registrar.submit: covariance_mode needs %s" % what)
            assert cov36_dev.numel() >= 36 * n and cov_flags_dev.numel() >= n
            _check(lib().ndtgpu_register_batch_cov_device(*args, int(covariance_mode), C.c_void_p(cov36_dev.data_ptr()),
                                                          C.c_void_p(cov_flags_dev.data_ptr()), _stream_ptr(stream), C.byref(t)))
        return int(t.value)

    def register_host(self, targets, sources, T, range_limit=-1.0, n_min=3, eval_factor=1000.0, covariance_mode=None, **params):
        """Host form: targets / sources NumPy float32 [n, N, 3 or 4], T [n, 4, 4] initial guesses -> (T [n, 4, 4], results);
        with covariance_mode 0 / 1 (ndtgpu_register_batch_cov_host) -> (T, results, cov [n, 6, 6], flags [n] int32 COV_*)."""
        tg = np.ascontiguousarray(targets, dtype=np.float32)
        sc = np.ascontiguousarray(sources, dtype=np.float32)
        n, npts, w = tg.shape
        assert sc.shape == tg.shape and w in (3, 4)
        Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
        res = np.zeros(n, dtype=RESULT_DTYPE)
        cp = CellParams(int(n_min), float(eval_factor))
        p = match_params(**params)
        args = (self.h, C.c_void_p(tg.ctypes.data), C.c_void_p(sc.ctypes.data), npts, 4 * w, 4 * w * npts, float(range_limit),
                C.byref(cp), _dp(Tc), n, C.byref(p), C.c_void_p(res.ctypes.data))
        if covariance_mode is None:
            _check(lib().ndtgpu_register_batch_host(*args))
            return np.transpose(Tc.reshape(n, 4, 4), (0, 2, 1)).copy(), res
        cov = np.zeros((n, 36), dtype=np.float64)
        flags = np.zeros(n, dtype=np.int32)
        _check(lib().ndtgpu_register_batch_cov_host(*args, int(covariance_mode), _dp(cov), flags.ctypes.data_as(C.POINTER(C.c_int32))))
        return np.transpose(Tc.reshape(n, 4, 4), (0, 2, 1)).copy(), res, cov.reshape(n, 6, 6), flags

    def wait_stream(self, stream=None, ticket=0):
        """`stream` waits for the call `ticket` names (0: for everything submitted so far); the host does not wait."""
        _check(lib().ndtgpu_registrar_wait_stream(self.h, int(ticket), _stream_ptr(stream)))

    def sync(self):
        _check(lib().ndtgpu_registrar_sync(self.h))

    def profiling(self, on=True):
        _check(lib().ndtgpu_registrar_profiling(self.h, 1 if on else 0))

    def kernel_ms(self):
        """-> (mean build ms, mean matcher ms, profiled sub-batches) since the last call; forgets them."""
        ms = (C.c_float * 2)()
        n = C.c_int32()
        _check(lib().ndtgpu_registrar_kernel_ms(self.h, ms, C.byref(n)))
        return float(ms[0]), float(ms[1]), int(n.value)

    def mapset(self, slot):
        h = C.c_void_p()
        _check(lib().ndtgpu_registrar_mapset(self.h, int(slot), C.byref(h)))
        return _BorrowedMapSet(h, 2 * self.per, self.res)


MAX_LEVELS = 8      # NDTGPU_MAX_LEVELS


class MultiResInfo(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("pairs_per_batch", C.c_size_t), ("levels_fused", C.c_uint64), ("levels_unfused", C.c_uint64)]


def default_resolutions():
    """NDTMatcherD2D's default list (ndtgpu_default_resolutions): (0.2, 0.5, 1.0, 2.0)"""
    r = (C.c_double * 4)()
    n = C.c_int32()
    lib().ndtgpu_default_resolutions(r, C.byref(n))
    return tuple(r[:n.value])


class MultiRes(_Handle):
    """ndtgpu_multires: NDTMatcherD2D(irregular, useDefaultGridResolutions, resolutions).match(target_pc, source_pc, T,
    useInitialGuess) -- coarse-to-fine D2D registration of raw scan pairs, sub-batch after sub-batch of pairs_per_batch
    (include/ndtgpu.h).  Every level's maps sit on the grid (centre, size_m) at the level's cell size; resolutions=None: the
    default list.  The levels run from the last entry of the list to the first."""
    _destroy = "ndtgpu_multires_destroy"

    def __init__(self, centre, size_m, resolutions=None, pairs_per_batch=1024, max_cells=0):
        gp = GridParams()
        gp.res = 0.0                                   # (ignored: each level has its own)
        gp.centre[:] = [float(x) for x in centre]
        gp.size[:] = [float(x) for x in size_m]
        gp.max_cells = int(max_cells)
        res = default_resolutions() if resolutions is None else tuple(float(r) for r in resolutions)
        arr = (C.c_double * max(1, len(res)))(*res)
        h = C.c_void_p()
        _check(lib().ndtgpu_multires_create(C.byref(gp), arr, len(res), int(pairs_per_batch), C.byref(h)))
        self.h, self.resolutions, self.per = h, res, int(pairs_per_batch)

    @property
    def n_levels(self):
        return len(self.resolutions)

    def info(self):
        """ndtgpu_multires_get_info: n_levels, pairs_per_batch, and the source builds so far that moved the clouds on load
        (levels_fused) or before a separate build (levels_unfused)"""
        i = MultiResInfo()
        _check(lib().ndtgpu_multires_get_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in MultiResInfo._fields_}

    def register_device(self, targets, sources, T16_dev, results_dev, use_initial_guess=True, range_limit=-1.0, n_min=3,
                        eval_factor=1000.0, stream=None, **params):
        """targets / sources: torch CUDA float32 [n, N, 3 or 4] (contiguous in the last two dims); T16_dev float64 [n, 16]
        column-major (in: initial guess, out: pose); results_dev uint8 [n, n_levels * 64] (result of pair k at list position j:
        record k * n_levels + j).  Asynchronous on `stream`."""
        n, npts = int(targets.shape[0]), int(targets.shape[1])
        assert tuple(sources.shape) == tuple(targets.shape) and targets.stride(1) == targets.shape[2] and targets.stride(2) == 1
        assert sources.stride(0) == targets.stride(0) and sources.stride(1) == targets.stride(1) and sources.stride(2) == 1
        assert T16_dev.numel() >= 16 * n and results_dev.numel() >= 64 * n * self.n_levels
        cp = CellParams(int(n_min), float(eval_factor))
        p = match_params(**params)
        _check(lib().ndtgpu_register_multires_device(self.h, C.c_void_p(targets.data_ptr()), C.c_void_p(sources.data_ptr()), npts,
                                                     4 * int(targets.shape[2]), 4 * int(targets.stride(0)), float(range_limit),
                                                     C.byref(cp), C.c_void_p(T16_dev.data_ptr()), n, C.byref(p),
                                                     1 if use_initial_guess else 0, C.c_void_p(results_dev.data_ptr()),
                                                     _stream_ptr(stream)))

    def register_host(self, targets, sources, T, use_initial_guess=True, range_limit=-1.0, n_min=3, eval_factor=1000.0, **params):
        """Host form: targets / sources NumPy float32 [n, N, 3 or 4], T [n, 4, 4] initial guesses -> (T [n, 4, 4],
        results [n, n_levels] RESULT_DTYPE, in list order)."""
        tg = np.ascontiguousarray(targets, dtype=np.float32)
        sc = np.ascontiguousarray(sources, dtype=np.float32)
        n, npts, w = tg.shape
        assert sc.shape == tg.shape and w in (3, 4)
        Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
        res = np.zeros(n * self.n_levels, dtype=RESULT_DTYPE)
        cp = CellParams(int(n_min), float(eval_factor))
        p = match_params(**params)
        _check(lib().ndtgpu_register_multires_host(self.h, C.c_void_p(tg.ctypes.data), C.c_void_p(sc.ctypes.data), npts, 4 * w,
                                                   4 * w * npts, float(range_limit), C.byref(cp), _dp(Tc), n, C.byref(p),
                                                   1 if use_initial_guess else 0, C.c_void_p(res.ctypes.data)))
        return np.transpose(Tc.reshape(n, 4, 4), (0, 2, 1)).copy(), res.reshape(n, self.n_levels)


class MclParams(C.Structure):
    _fields_ = [("map_res", C.c_double), ("sensor_res", C.c_double), ("scan_size", C.c_double * 3), ("range_limit", C.c_double),
                ("zfilt_min", C.c_double), ("motion_model", C.c_double * 36), ("motion_model_offset", C.c_double * 6),
                ("force_sir", C.c_int32), ("sir_max_iters_wo_resampling", C.c_int32), ("sir_varp_threshold", C.c_double),
                ("max_scan_cells", C.c_uint32), ("pad_", C.c_uint32), ("seed", C.c_uint64)]


class MclResult(C.Structure):
    _fields_ = [("var_p", C.c_double), ("lik_sum", C.c_double), ("terms", C.c_int64), ("draws", C.c_uint64), ("resampled", C.c_int32),
                ("since_sir", C.c_int32), ("n_scan_cells", C.c_int32), ("overflow", C.c_int32)]


MCL_RESULT_DTYPE = np.dtype([("var_p", "<f8"), ("lik_sum", "<f8"), ("terms", "<i8"), ("draws", "<u8"), ("resampled", "<i4"),
                             ("since_sir", "<i4"), ("n_scan_cells", "<i4"), ("overflow", "<i4")])
assert MCL_RESULT_DTYPE.itemsize == C.sizeof(MclResult)


def mcl_params(**fields):
    """ndtgpu_default_mcl_params with fields replaced (motion_model: 36 values row-major, scan_size / motion_model_offset: 3 / 6)"""
    return _params(MclParams, "ndtgpu_default_mcl_params", "MCL", fields)


class MCL(_Handle):
    """ndtgpu_mcl: a bank of n_filters NDTMCL3D particle filters of n_particles particles; filter k localises in map map_idx[k]
    of the borrowed MapSet map_set (include/ndtgpu.h).  Poses are 4x4 (math convention) in and out."""
    _destroy = "ndtgpu_mcl_destroy"

    def __init__(self, map_set, map_idx, n_particles, **params):
        idx = np.ascontiguousarray(np.atleast_1d(map_idx), dtype=np.uint32)
        p = mcl_params(**params)
        h = C.c_void_p()
        _check(lib().ndtgpu_mcl_create(map_set.h, idx.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(p), idx.shape[0], int(n_particles),
                                       C.byref(h)))
        self.h, self.map_set, self.n_filters, self.n_particles = h, map_set, int(idx.shape[0]), int(n_particles)

    @staticmethod
    def _cm(T, n):
        """[n, 4, 4] math convention -> [n, 16] column-major"""
        return np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).reshape(n, 16)

    def initialize(self, pose6, sigma6, first=0):
        """initializeFilter(x, y, z, r, p, t, sx, sy, sz, sr, sp, st) for filters [first, first + count): pose6 / sigma6 [count, 6]"""
        ps, sg = _f64(pose6).reshape(-1, 6), _f64(sigma6).reshape(-1, 6)
        assert ps.shape == sg.shape
        _check(lib().ndtgpu_mcl_initialize(self.h, int(first), ps.shape[0], _dp(ps), _dp(sg)))

    def set_particles(self, T, weights=None, first=0):
        """pf.pcloud[i].T / .p: T [count, N, 4, 4], weights [count, N] (None: 1/N)"""
        T = np.asarray(T, dtype=np.float64)
        n = int(T.size // 16)
        if T.size != 16 * n or n == 0 or n % self.n_particles:
            raise ValueError("set_particles: T must hold whole sets of n_particles 4 x 4 poses")
        count = n // self.n_particles
        Tc = self._cm(T, n)
        w = None
        if weights is not None:
            w = _f64(weights)
            if w.size != n:
                raise ValueError("set_particles: weights must hold one value per particle")
            w = w.reshape(n)
        _check(lib().ndtgpu_mcl_set_particles(self.h, int(first), count, _dp(Tc), None if w is None else _dp(w)))

    def update(self, Tmotion, xyz, subsample_level=1.0, first=0, stream=None):
        """updateAndPredictEff(Tmotion, cloud, subsample_level) for filters [first, first + count): Tmotion [count, 4, 4]; xyz [count, N,
        3 or 4] float32 in the base frame -- a torch CUDA tensor (asynchronous on `stream`) or a NumPy array (host path, synchronous)"""
        if xyz.ndim == 2:
            xyz = xyz[None]
        count, npts, w = int(xyz.shape[0]), int(xyz.shape[1]), int(xyz.shape[2])
        assert w in (3, 4)
        Tm = self._cm(Tmotion, count)
        if hasattr(xyz, "data_ptr"):
            import torch
            assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.is_contiguous()
            if stream is None:
                stream = torch.cuda.current_stream()
            _check(lib().ndtgpu_mcl_update(self.h, int(first), count, _dp(Tm), float(subsample_level), C.c_void_p(xyz.data_ptr()), npts,
                                           4 * w, 4 * w * npts, _stream_ptr(stream)))
        else:
            a = np.ascontiguousarray(xyz, dtype=np.float32)
            _check(lib().ndtgpu_mcl_update_host(self.h, int(first), count, _dp(Tm), float(subsample_level), C.c_void_p(a.ctypes.data),
                                                npts, 4 * w, 4 * w * npts))

    def particles(self, first=0, count=None):
        """(T [count, N, 4, 4], weights [count, N], lik [count, N]) of filters [first, first + count)"""
        count = self.n_filters - first if count is None else int(count)
        n = count * self.n_particles
        T = np.zeros((n, 16))
        w = np.zeros(n)
        lik = np.zeros(n)
        _check(lib().ndtgpu_mcl_particles(self.h, int(first), count, _dp(T), _dp(w), _dp(lik)))
        T = np.transpose(T.reshape(n, 4, 4), (0, 2, 1)).reshape(count, self.n_particles, 4, 4)
        return T, w.reshape(count, self.n_particles), lik.reshape(count, self.n_particles)

    def particle_markers(self, first=0, count=None, out=None, stream=None, **params):
        """markerParticlesNDTMCL3D of filters [first, first + count) (ndtgpu_mcl_markers): per particle its position and the point
        particle_length (0.3) along its x axis -> points [count, N, 2, 3].  out: a float64 torch device tensor of count * N * 6
        elements takes the device form (asynchronous on `stream`) and is returned reshaped."""
        count = self.n_filters - first if count is None else int(count)
        p = marker_params(**params)
        n = count * self.n_particles
        if out is not None:
            import torch
            _check(lib().ndtgpu_mcl_markers_device(self.h, int(first), count, C.byref(p),
                                                   _dev_ptr(out, torch.float64, 6 * n, "MCL.particle_markers out"), _stream_ptr(stream)))
            return out.view(-1)[:6 * n].view(count, self.n_particles, 2, 3)
        pts = np.zeros((max(n, 1), 6))
        _check(lib().ndtgpu_mcl_markers(self.h, int(first), count, C.byref(p), _dp(pts)))
        return pts[:n].reshape(count, self.n_particles, 2, 3)

    def mean(self, first=0, count=None):
        """pf.getMean() [count, 4, 4] and the last update's records (MCL_RESULT_DTYPE [count])"""
        count = self.n_filters - first if count is None else int(count)
        T = np.zeros((count, 16))
        res = np.zeros(count, dtype=MCL_RESULT_DTYPE)
        _check(lib().ndtgpu_mcl_mean(self.h, int(first), count, _dp(T), C.c_void_p(res.ctypes.data)))
        return np.transpose(T.reshape(count, 4, 4), (0, 2, 1)).copy(), res


class PgoParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_linear_iterations", C.c_int32), ("eps_step", C.c_double), ("eps_linear", C.c_double),
                ("prior_information", C.c_double * 9)]


class PgoResult(C.Structure):
    _fields_ = [("exit_code", C.c_int32), ("iterations", C.c_int32), ("linear_iterations", C.c_int32), ("pad_", C.c_int32),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("max_step", C.c_double), ("n_nodes", C.c_int32),
                ("n_edges", C.c_int32)]


class PgoWideParams(C.Structure):
    _fields_ = [("check_every", C.c_int32), ("pad_", C.c_int32)]


# ndtgpu_pgo_result.exit_code (include/ndtgpu.h NDTGPU_PGO_*)
PGO_CONVERGED, PGO_MAX_ITERATIONS, PGO_LINEAR_CAP, PGO_NOT_FINITE = 0, 1, 2, 3


def pgo_params(**fields):
    """ndtgpu_default_pgo_params with fields replaced (prior_information: 9 values row-major)"""
    return _params(PgoParams, "ndtgpu_default_pgo_params", "PGO", fields)


def pgo_wide_params(check_every=None):
    """ndtgpu_default_pgo_wide_params, check_every replaced where given"""
    p = PgoWideParams()
    lib().ndtgpu_default_pgo_wide_params(C.byref(p))
    if check_every is not None:
        p.check_every = int(check_every)
    return p


def pgo_wide_plan(n_nodes, n_edges):
    """ndtgpu_pgo_wide_plan -> (tile, node tiles, link tiles, extra device bytes) of a graph of this size"""
    tile, nt, et, extra = C.c_uint32(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    _check(lib().ndtgpu_pgo_wide_plan(int(n_nodes), int(n_edges), C.byref(tile), C.byref(nt), C.byref(et), C.byref(extra)))
    return tile.value, nt.value, et.value, extra.value


class PgoMarginalParams(C.Structure):
    _fields_ = [("max_workspace_bytes", C.c_uint64)]


class PgoMarginalResult(C.Structure):
    _fields_ = [("exit_code", C.c_int32), ("linear_iterations", C.c_int32), ("max_column_iterations", C.c_int32),
                ("capped_columns", C.c_int32), ("asymmetry", C.c_double)]


# ndtgpu_pgo_marginal_result as a NumPy record: what marginals() returns per query, and how to read a results_dev buffer
PGO_MARGINAL_RESULT = np.dtype([("exit_code", np.int32), ("linear_iterations", np.int32), ("max_column_iterations", np.int32),
                                ("capped_columns", np.int32), ("asymmetry", np.float64)])


def pgo_marginal_params(max_workspace_bytes=None):
    """ndtgpu_default_pgo_marginal_params, max_workspace_bytes replaced where given"""
    p = PgoMarginalParams()
    lib().ndtgpu_default_pgo_marginal_params(C.byref(p))
    if max_workspace_bytes is not None:
        p.max_workspace_bytes = int(max_workspace_bytes)
    return p


def pgo_marginal_plan(max_nodes, max_edges, n_queries, dof, max_workspace_bytes=None):
    """ndtgpu_pgo_marginal_plan (pure host) -> (slot bytes, slots, solve launches) of a marginals call on a bank of this capacity;
    dof 3: PGO, 6: PGO3; max_workspace_bytes None: the default budget"""
    sb, sl, la = C.c_size_t(), C.c_size_t(), C.c_size_t()
    budget = pgo_marginal_params(max_workspace_bytes).max_workspace_bytes
    _check(lib().ndtgpu_pgo_marginal_plan(int(max_nodes), int(max_edges), int(n_queries), int(dof), budget, C.byref(sb), C.byref(sl), C.byref(la)))
    return sb.value, sl.value, la.value


def pgo_relative_covariance(pose_ref, pose_mov, cov_ref, cov_mov, cross):
    """ndtgpu_pgo_relative_covariance (pure host): the 3x3 covariance of the error of a link ref -> mov at the current relative
    pose; poses (x, y, yaw), cross = the block [mov, ref] (marginals with node = ref, other = mov)"""
    out = np.zeros((3, 3))
    _check(lib().ndtgpu_pgo_relative_covariance(_dp(_f64(pose_ref).reshape(3)), _dp(_f64(pose_mov).reshape(3)), _dp(_f64(cov_ref).reshape(9)),
                                                _dp(_f64(cov_mov).reshape(9)), _dp(_f64(cross).reshape(9)), _dp(out)))
    return out


def pgo3_relative_covariance(T_ref, T_mov, cov_ref, cov_mov, cross):
    """ndtgpu_pgo3_relative_covariance (pure host): the 6x6 covariance of the error of a link ref -> mov at the current relative
    pose; poses 4x4, cross = the block [mov, ref]"""
    out = np.zeros((6, 6))
    _check(lib().ndtgpu_pgo3_relative_covariance(_dp(_cm16(T_ref)), _dp(_cm16(T_mov)), _dp(_f64(cov_ref).reshape(36)),
                                                 _dp(_f64(cov_mov).reshape(36)), _dp(_f64(cross).reshape(36)), _dp(out)))
    return out


class PgoRobustParams(C.Structure):
    _fields_ = [("kind", C.c_int32), ("max_rounds", C.c_int32), ("updates_per_round", C.c_int32), ("min_index_gap", C.c_int32),
                ("scale", C.c_double), ("inlier_weight", C.c_double)]


class PgoRobustResult(C.Structure):
    _fields_ = [("exit_code", C.c_int32), ("rounds", C.c_int32), ("updates", C.c_int32), ("linear_iterations", C.c_int32),
                ("cost_initial", C.c_double), ("cost_final", C.c_double), ("chi2_final", C.c_double), ("outliers", C.c_int32),
                ("pad_", C.c_int32)]


assert C.sizeof(PgoRobustParams) == 32 and C.sizeof(PgoRobustResult) == 48

# ndtgpu_pgo_robust_params.kind (include/ndtgpu.h NDTGPU_PGO_ROBUST_*); PGO_MAX_ROUNDS: ndtgpu_pgo_robust_result.exit_code, the
# slot of PGO_MAX_ITERATIONS
PGO_ROBUST_HUBER, PGO_ROBUST_CAUCHY, PGO_ROBUST_DCS = 1, 2, 3
PGO_MAX_ROUNDS = PGO_MAX_ITERATIONS
_PGO_ROBUST_KINDS = {"huber": PGO_ROBUST_HUBER, "cauchy": PGO_ROBUST_CAUCHY, "dcs": PGO_ROBUST_DCS}


def _pgo_robust_kind(kind):
    return _PGO_ROBUST_KINDS[kind.lower()] if isinstance(kind, str) else int(kind)


def pgo_robust_params(**fields):
    """ndtgpu_default_pgo_robust_params with fields replaced; kind: PGO_ROBUST_* or "huber" / "cauchy" / "dcs" """
    if "kind" in fields:
        fields = dict(fields, kind=_pgo_robust_kind(fields["kind"]))
    return _params(PgoRobustParams, "ndtgpu_default_pgo_robust_params", "PGO robust", fields)


def pgo_robust_weight(kind, scale, chi2):
    """ndtgpu_pgo_robust_weight (pure host): the weights of links from their chi2 (a number or an array), the device's bits"""
    x = np.asarray(chi2, dtype=np.float64)
    out = np.empty(x.size)
    w = C.c_double()
    for k, v in enumerate(x.ravel()):
        _check(lib().ndtgpu_pgo_robust_weight(_pgo_robust_kind(kind), float(scale), float(v), C.byref(w)))
        out[k] = w.value
    return out.reshape(x.shape) if x.ndim else float(out[0])


class _Robust:
    """optimize_robust / robust_links / robust_restore of the two pose-graph banks (include/ndtgpu.h: robust loop-closure weighting);
    _robust_fn, _robust_links_fn, _robust_restore_fn and _params_fn are the bank's"""

    def optimize_robust(self, first=0, count=None, robust=None, wide=False, check_every=None, stream=None, **params):
        """graphs [first, first + count) by iteratively re-weighted least squares round optimize (wide: optimize_wide, one graph);
        returns when every graph has stopped.  robust: a dict of ndtgpu_pgo_robust_params fields or a PgoRobustParams (None: the
        defaults); keyword arguments: fields of the bank's params.  The bank is left weighted: robust_restore(g) puts the
        information as set back."""
        count = self.n_graphs - first if count is None else int(count)
        p = self._params_fn(**params)
        rp = robust if isinstance(robust, PgoRobustParams) else pgo_robust_params(**(robust or {}))
        w = pgo_wide_params(check_every) if wide else None
        _check(getattr(lib(), self._robust_fn)(self.h, int(first), count, C.byref(p), C.byref(rp), None if w is None else C.byref(w),
                                               _stream_ptr(stream)))

    def robust_links(self, g):
        """(chi2 [m], weight [m], inlier [m] bool, result dict) of graph g's m links as the last robust call left them"""
        m = self._n_edges[int(g)]
        chi2, weight, inlier = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(max(m, 1), dtype=np.int32)
        r = PgoRobustResult()
        _check(getattr(lib(), self._robust_links_fn)(self.h, int(g), _dp(chi2), _dp(weight), inlier.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(r)))
        return chi2[:m], weight[:m], inlier[:m] != 0, {k: getattr(r, k) for k, _ in PgoRobustResult._fields_ if k != "pad_"}

    def information(self, g):
        """[m, 6] (PGO) or [m, 21] (PGO3): graph g's information as the bank holds it, in the bank's layout (include/ndtgpu.h)"""
        m, k = self._n_edges[int(g)], 6 if self._dof == 3 else 21
        out = np.zeros((max(m, 1), k))
        _check(getattr(lib(), self._information_fn)(self.h, int(g), _dp(out)))
        return out[:m]

    def robust_restore(self, g):
        """the information as graph g was set back into the bank"""
        _check(getattr(lib(), self._robust_restore_fn)(self.h, int(g)))


class _Marginals:
    """marginals / marginals_device of the two pose-graph banks (include/ndtgpu.h: marginal covariances); _dof, _marginals_fn,
    _marginals_device_fn and _params_fn are the bank's"""

    def _marginal_queries(self, graph_idx, node_idx, other_idx):
        u32p = C.POINTER(C.c_uint32)
        ni = np.ascontiguousarray(node_idx, dtype=np.uint32).reshape(-1)
        gi = np.ascontiguousarray(np.broadcast_to(np.asarray(graph_idx, dtype=np.uint32), ni.shape))
        oi = None if other_idx is None else np.ascontiguousarray(other_idx, dtype=np.uint32).reshape(-1)
        if oi is not None and oi.shape != ni.shape:
            raise ValueError("marginals: one other node per query")
        return gi, ni, oi, gi.ctypes.data_as(u32p), ni.ctypes.data_as(u32p), None if oi is None else oi.ctypes.data_as(u32p)

    def marginals(self, graph_idx, node_idx, other_idx=None, max_workspace_bytes=None, **params):
        """(cov [n, dof, dof], cross [n, dof, dof] or None, results: PGO_MARGINAL_RESULT records [n]) of the queries (graph_idx: one
        index or one per query; other_idx None: no cross blocks) at the poses the graphs hold; keyword arguments: fields of the
        bank's params, of which prior_information -- the one the graph was optimised with --, eps_linear and max_linear_iterations
        are read.  Waits for the result."""
        gi, ni, oi, gp, np_, op = self._marginal_queries(graph_idx, node_idx, other_idx)
        n, d = ni.shape[0], self._dof
        cov = np.zeros((n, d, d))
        cross = None if oi is None else np.zeros((n, d, d))
        res = np.zeros(n, dtype=PGO_MARGINAL_RESULT)
        p, mp = self._params_fn(**params), pgo_marginal_params(max_workspace_bytes)
        _check(getattr(lib(), self._marginals_fn)(self.h, n, gp, np_, op, C.byref(p), C.byref(mp), _dp(cov), None if cross is None else _dp(cross),
                                                  res.ctypes.data_as(C.POINTER(PgoMarginalResult))))
        return cov, cross, res

    def marginals_device(self, graph_idx, node_idx, other_idx, cov_dev, cross_dev, results_dev, stream=None, max_workspace_bytes=None, **params):
        """the same into torch CUDA tensors, asynchronous on `stream`: cov_dev (and cross_dev unless other_idx is None) float64 with
        n * dof * dof elements, results_dev uint8 with n * 24 bytes (read back: .cpu().numpy().view(PGO_MARGINAL_RESULT))"""
        gi, ni, oi, gp, np_, op = self._marginal_queries(graph_idx, node_idx, other_idx)
        n, d = ni.shape[0], self._dof
        assert cov_dev.is_cuda and cov_dev.is_contiguous() and cov_dev.numel() * cov_dev.element_size() >= 8 * n * d * d
        assert results_dev.is_cuda and results_dev.is_contiguous() and results_dev.numel() * results_dev.element_size() >= n * PGO_MARGINAL_RESULT.itemsize
        if oi is not None:
            assert cross_dev.is_cuda and cross_dev.is_contiguous() and cross_dev.numel() * cross_dev.element_size() >= 8 * n * d * d
        p, mp = self._params_fn(**params), pgo_marginal_params(max_workspace_bytes)
        _check(getattr(lib(), self._marginals_device_fn)(self.h, n, gp, np_, op, C.byref(p), C.byref(mp), C.c_void_p(cov_dev.data_ptr()),
                                                         None if oi is None else C.c_void_p(cross_dev.data_ptr()),
                                                         C.c_void_p(results_dev.data_ptr()), _stream_ptr(stream)))


class PGO(_Handle, _Marginals, _Robust):
    """ndtgpu_pgo: a bank of n_graphs SE(2) pose graphs of up to max_nodes nodes and max_edges links, optimised one workgroup per
    graph (include/ndtgpu.h: optimizeGraphUsingISAM).  Poses are (x, y, yaw) rows."""
    _destroy = "ndtgpu_pgo_destroy"
    _dof, _marginals_fn, _marginals_device_fn, _params_fn = 3, "ndtgpu_pgo_marginals", "ndtgpu_pgo_marginals_device", staticmethod(pgo_params)
    _robust_fn, _robust_links_fn, _robust_restore_fn = "ndtgpu_pgo_optimize_robust", "ndtgpu_pgo_robust_links", "ndtgpu_pgo_robust_restore"
    _information_fn = "ndtgpu_pgo_link_information"

    def __init__(self, n_graphs, max_nodes, max_edges):
        h = C.c_void_p()
        _check(lib().ndtgpu_pgo_create(int(n_graphs), int(max_nodes), int(max_edges), C.byref(h)))
        self.h, self.n_graphs = h, int(n_graphs)
        self._n_nodes, self._n_edges = [0] * int(n_graphs), [0] * int(n_graphs)

    @staticmethod
    def _graph(poses, ref, mov):
        ps = _f64(poses).reshape(-1, 3)
        ri = np.ascontiguousarray(ref, dtype=np.uint32).reshape(-1)
        mi = np.ascontiguousarray(mov, dtype=np.uint32).reshape(-1)
        if ri.shape != mi.shape:
            raise ValueError("PGO: one ref and one mov index per link")
        u32p = C.POINTER(C.c_uint32)
        return ps, ri, mi, ri.ctypes.data_as(u32p), mi.ctypes.data_as(u32p)

    def set_graph(self, g, poses, ref, mov, meas, info=None):
        """graph g: poses [n, 3] (node 0's is the prior's origin), links ref -> mov with meas [m, 3] and info [m, 3, 3] (None: 100 I)"""
        ps, ri, mi, rp, mp = self._graph(poses, ref, mov)
        z = _f64(meas).reshape(-1, 3)
        W = None if info is None else _f64(info).reshape(-1, 9)
        if z.shape[0] != ri.shape[0] or (W is not None and W.shape[0] != ri.shape[0]):
            raise ValueError("PGO.set_graph: one measurement (and information matrix) per link")
        _check(lib().ndtgpu_pgo_set_graph(self.h, int(g), ps.shape[0], _dp(ps), ri.shape[0], rp, mp, _dp(z), None if W is None else _dp(W)))
        self._n_nodes[int(g)], self._n_edges[int(g)] = ps.shape[0], ri.shape[0]

    def set_links_device(self, g, poses, ref, mov, T16_dev, cov36_dev=None, cov_flags_dev=None):
        """graph g with its links as ndtgpu_register_batch_cov_device left them: torch CUDA tensors T16_dev float64 [m, 16],
        cov36_dev float64 [m, 36] and cov_flags_dev int32 [m] (both None: 100 I for every link), complete when the call is made"""
        ps, ri, mi, rp, mp = self._graph(poses, ref, mov)
        m = ri.shape[0]
        assert T16_dev.is_cuda and T16_dev.is_contiguous() and T16_dev.numel() >= 16 * m
        if cov36_dev is not None:
            assert cov36_dev.is_cuda and cov36_dev.is_contiguous() and cov36_dev.numel() >= 36 * m
            assert cov_flags_dev is not None and cov_flags_dev.is_cuda and cov_flags_dev.numel() >= m
        _check(lib().ndtgpu_pgo_set_links_device(self.h, int(g), ps.shape[0], _dp(ps), m, rp, mp, C.c_void_p(T16_dev.data_ptr()),
                                                 None if cov36_dev is None else C.c_void_p(cov36_dev.data_ptr()),
                                                 None if cov36_dev is None else C.c_void_p(cov_flags_dev.data_ptr())))
        self._n_nodes[int(g)], self._n_edges[int(g)] = ps.shape[0], ri.shape[0]

    def optimize(self, first=0, count=None, stream=None, **params):
        """graphs [first, first + count) in one launch, asynchronous on `stream`; keyword arguments: fields of ndtgpu_pgo_params"""
        count = self.n_graphs - first if count is None else int(count)
        p = pgo_params(**params)
        _check(lib().ndtgpu_pgo_optimize(self.h, int(first), count, C.byref(p), _stream_ptr(stream)))

    def optimize_wide(self, g, stream=None, check_every=None, **params):
        """graph g alone, spread over the device (ndtgpu_pgo_optimize_wide): returns when the graph is done; check_every: inner
        iterations enqueued between two looks at the control block (None: the default); keyword arguments: fields of ndtgpu_pgo_params"""
        p, w = pgo_params(**params), pgo_wide_params(check_every)
        _check(lib().ndtgpu_pgo_optimize_wide(self.h, int(g), C.byref(p), C.byref(w), _stream_ptr(stream)))

    def poses(self, g, with_T=False):
        """(poses [n, 3], result dict) of graph g, with_T: (poses, T [n, 4, 4], result); waits for the handle"""
        n = self._n_nodes[int(g)]
        ps = np.zeros((max(n, 1), 3))
        T = np.zeros((max(n, 1), 16)) if with_T else None
        r = PgoResult()
        _check(lib().ndtgpu_pgo_poses(self.h, int(g), _dp(ps), None if T is None else _dp(T), C.byref(r)))
        res = {k: getattr(r, k) for k, _ in PgoResult._fields_ if k != "pad_"}
        if with_T:
            return ps, np.transpose(T.reshape(-1, 4, 4), (0, 2, 1)).copy(), res
        return ps, res


class Pgo3Params(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_linear_iterations", C.c_int32), ("eps_step", C.c_double), ("eps_linear", C.c_double),
                ("prior_information", C.c_double * 36)]


PGO3_HALF_TURN = 4    # ndtgpu_pgo_result.exit_code beside PGO_* (include/ndtgpu.h NDTGPU_PGO3_HALF_TURN)


def pgo3_params(**fields):
    """ndtgpu_default_pgo3_params with fields replaced (prior_information: 36 values row-major)"""
    return _params(Pgo3Params, "ndtgpu_default_pgo3_params", "PGO3", fields)


def _cm16(T):
    """poses [n, 4, 4] as the ABI's column-major T16 rows [n, 16]"""
    return np.ascontiguousarray(np.transpose(_f64(T).reshape(-1, 4, 4), (0, 2, 1))).reshape(-1, 16)


def _from_cm16(T16):
    return np.transpose(T16.reshape(-1, 4, 4), (0, 2, 1)).copy()


def pgo3_link_error(Ti, Tj, Z):
    """ndtgpu_pgo3_link_error (pure host) -> (e [6], J_ref [6, 6], J_mov [6, 6]) of a link ref = Ti, mov = Tj, all 4x4"""
    e, Jr, Jm = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    _check(lib().ndtgpu_pgo3_link_error(_dp(_cm16(Ti)), _dp(_cm16(Tj)), _dp(_cm16(Z)), _dp(e), _dp(Jr), _dp(Jm)))
    return e, Jr, Jm


def pgo3_retract(T, d):
    """ndtgpu_pgo3_retract (pure host): T [+] d, d = (rho, phi) -> 4x4"""
    out = np.zeros((1, 16))
    _check(lib().ndtgpu_pgo3_retract(_dp(_cm16(T)), _dp(_f64(d).reshape(6)), _dp(out)))
    return _from_cm16(out)[0]


def pgo3_link_from_registration(T, cov36=None, flags=0):
    """ndtgpu_pgo3_link_from_registration (pure host) -> (Z [4, 4], W [6, 6]) of one registered link: T 4x4, cov36 row-major 6x6"""
    Z, W = np.zeros((1, 16)), np.zeros((6, 6))
    c = None if cov36 is None else _f64(cov36).reshape(36)
    _check(lib().ndtgpu_pgo3_link_from_registration(_dp(_cm16(T)), None if c is None else _dp(c), int(flags), _dp(Z), _dp(W)))
    return _from_cm16(Z)[0], W


def pgo3_wide_plan(n_nodes, n_edges):
    """ndtgpu_pgo3_wide_plan -> (tile, node tiles, link tiles, extra device bytes) of a graph of this size; the link tiles count
    the prior, the link behind the last"""
    tile, nt, lt, extra = C.c_uint32(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    _check(lib().ndtgpu_pgo3_wide_plan(int(n_nodes), int(n_edges), C.byref(tile), C.byref(nt), C.byref(lt), C.byref(extra)))
    return tile.value, nt.value, lt.value, extra.value


class PGO3(_Handle, _Marginals, _Robust):
    """ndtgpu_pgo3: a bank of n_graphs SE(3) pose graphs of up to max_nodes nodes and max_edges links, optimised one workgroup per
    graph (include/ndtgpu.h: SE(3) pose-graph optimisation).  Poses are 4x4 matrices [n, 4, 4]."""
    _destroy = "ndtgpu_pgo3_destroy"
    _dof, _marginals_fn, _marginals_device_fn, _params_fn = 6, "ndtgpu_pgo3_marginals", "ndtgpu_pgo3_marginals_device", staticmethod(pgo3_params)
    _robust_fn, _robust_links_fn, _robust_restore_fn = "ndtgpu_pgo3_optimize_robust", "ndtgpu_pgo3_robust_links", "ndtgpu_pgo3_robust_restore"
    _information_fn = "ndtgpu_pgo3_link_information"

    def __init__(self, n_graphs, max_nodes, max_edges):
        h = C.c_void_p()
        _check(lib().ndtgpu_pgo3_create(int(n_graphs), int(max_nodes), int(max_edges), C.byref(h)))
        self.h, self.n_graphs = h, int(n_graphs)
        self._n_nodes, self._n_edges = [0] * int(n_graphs), [0] * int(n_graphs)

    @staticmethod
    def _graph(poses, ref, mov):
        ps = _cm16(poses)
        ri = np.ascontiguousarray(ref, dtype=np.uint32).reshape(-1)
        mi = np.ascontiguousarray(mov, dtype=np.uint32).reshape(-1)
        if ri.shape != mi.shape:
            raise ValueError("PGO3: one ref and one mov index per link")
        u32p = C.POINTER(C.c_uint32)
        return ps, ri, mi, ri.ctypes.data_as(u32p), mi.ctypes.data_as(u32p)

    def set_graph(self, g, poses, ref, mov, meas, info=None):
        """graph g: poses [n, 4, 4] (node 0's is the prior's origin), links ref -> mov with meas [m, 4, 4] and info [m, 6, 6] (None:
        100 I)"""
        ps, ri, mi, rp, mp = self._graph(poses, ref, mov)
        z = _cm16(meas) if ri.shape[0] else np.zeros((0, 16))
        W = None if info is None else _f64(info).reshape(-1, 36)
        if z.shape[0] != ri.shape[0] or (W is not None and W.shape[0] != ri.shape[0]):
            raise ValueError("PGO3.set_graph: one measurement (and information matrix) per link")
        _check(lib().ndtgpu_pgo3_set_graph(self.h, int(g), ps.shape[0], _dp(ps), ri.shape[0], rp, mp, _dp(z), None if W is None else _dp(W)))
        self._n_nodes[int(g)], self._n_edges[int(g)] = ps.shape[0], ri.shape[0]

    def set_links_device(self, g, poses, ref, mov, T16_dev, cov36_dev=None, cov_flags_dev=None):
        """graph g with its links as ndtgpu_register_batch_cov_device left them: torch CUDA tensors T16_dev float64 [m, 16]
        (column-major), cov36_dev float64 [m, 36] and cov_flags_dev int32 [m] (both None: 100 I for every link), complete when the
        call is made"""
        ps, ri, mi, rp, mp = self._graph(poses, ref, mov)
        m = ri.shape[0]
        assert T16_dev.is_cuda and T16_dev.is_contiguous() and T16_dev.numel() >= 16 * m
        if cov36_dev is not None:
            assert cov36_dev.is_cuda and cov36_dev.is_contiguous() and cov36_dev.numel() >= 36 * m
            assert cov_flags_dev is not None and cov_flags_dev.is_cuda and cov_flags_dev.numel() >= m
        _check(lib().ndtgpu_pgo3_set_links_device(self.h, int(g), ps.shape[0], _dp(ps), m, rp, mp, C.c_void_p(T16_dev.data_ptr()),
                                                  None if cov36_dev is None else C.c_void_p(cov36_dev.data_ptr()),
                                                  None if cov36_dev is None else C.c_void_p(cov_flags_dev.data_ptr())))
        self._n_nodes[int(g)], self._n_edges[int(g)] = ps.shape[0], ri.shape[0]

    def optimize(self, first=0, count=None, stream=None, **params):
        """graphs [first, first + count) in one launch, asynchronous on `stream`; keyword arguments: fields of ndtgpu_pgo3_params"""
        count = self.n_graphs - first if count is None else int(count)
        p = pgo3_params(**params)
        _check(lib().ndtgpu_pgo3_optimize(self.h, int(first), count, C.byref(p), _stream_ptr(stream)))

    def optimize_wide(self, g, stream=None, check_every=None, **params):
        """graph g alone, spread over the device (ndtgpu_pgo3_optimize_wide): returns when the graph is done; check_every: inner
        iterations enqueued between two looks at the control block (None: the default); keyword arguments: fields of ndtgpu_pgo3_params"""
        p, w = pgo3_params(**params), pgo_wide_params(check_every)
        _check(lib().ndtgpu_pgo3_optimize_wide(self.h, int(g), C.byref(p), C.byref(w), _stream_ptr(stream)))

    def poses(self, g):
        """(poses [n, 4, 4], result dict) of graph g; waits for the handle"""
        T = np.zeros((max(self._n_nodes[int(g)], 1), 16))
        r = PgoResult()
        _check(lib().ndtgpu_pgo3_poses(self.h, int(g), _dp(T), C.byref(r)))
        return _from_cm16(T), {k: getattr(r, k) for k, _ in PgoResult._fields_ if k != "pad_"}


class WorldParams(C.Structure):
    _fields_ = [("maxnumpoints", C.c_double), ("eval_factor", C.c_double), ("occupancy_limit", C.c_double), ("reserved_", C.c_double * 2)]


class WorldResult(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_cells", C.c_int32), ("n_contributions", C.c_int64), ("n_dropped", C.c_int64),
                ("n_rejected", C.c_int64), ("n_points", C.c_int64), ("overflow", C.c_int32), ("s1_shift", C.c_int32),
                ("s2_shift", C.c_int32), ("pad_", C.c_int32)]


def world_params(**fields):
    """ndtgpu_default_world_params with fields replaced"""
    return _params(WorldParams, "ndtgpu_default_world_params", "world", fields, hidden=("reserved_",))


def assemble_world(dst, dst_first, src, node_lists, T16_lists, params=None, stream=None):
    """ndtgpu_world_assemble: destination maps dst_first, dst_first + 1, ... of `dst` become the worlds of node_lists -- world w
    merges the node maps node_lists[w] of `src` under the poses T16_lists[w] (4 x 4 matrices, node frame -> world frame).
    params: a WorldParams, a dict of its fields, or None.  Returns one dict per world (ndtgpu_world_result)."""
    count = len(node_lists)
    if len(T16_lists) != count:
        raise ValueError("assemble_world: one list of poses per world")
    off = np.zeros(count + 1, dtype=np.uint32)
    idx, Ts = [], []
    for w in range(count):
        nodes = [int(k) for k in node_lists[w]]
        T = _f64(T16_lists[w]).reshape(-1, 4, 4) if len(nodes) else np.zeros((0, 4, 4))
        if T.shape[0] != len(nodes):
            raise ValueError("assemble_world: one pose per listed node")
        idx += nodes
        Ts.append(np.transpose(T, (0, 2, 1)).reshape(-1, 16))           # column-major
        off[w + 1] = off[w] + len(nodes)
    idx = np.asarray(idx + [0], dtype=np.uint32)                        # (never an empty buffer)
    Tcm = np.ascontiguousarray(np.concatenate(Ts + [np.zeros((1, 16))], axis=0))
    if params is None or isinstance(params, WorldParams):
        p = params
    else:
        p = world_params(**dict(params))
    res = (WorldResult * max(count, 1))()
    u32p = C.POINTER(C.c_uint32)
    _check(lib().ndtgpu_world_assemble(dst.h, int(dst_first), count, src.h, off.ctypes.data_as(u32p), idx.ctypes.data_as(u32p), _dp(Tcm),
                                       None if p is None else C.byref(p), res, _stream_ptr(stream)))
    return [{k: getattr(res[w], k) for k, _ in WorldResult._fields_ if k != "pad_"} for w in range(count)]


class OccGridParams(C.Structure):
    _fields_ = [("z", C.c_double), ("occupied_no_gaussian", C.c_int32), ("reserved_", C.c_int32 * 5)]


class OccGridInfo(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("resolution", C.c_double), ("origin", C.c_double * 3),
                ("n_unknown", C.c_int64), ("n_free", C.c_int64), ("n_occupied", C.c_int64)]


def occgrid_params(**fields):
    """ndtgpu_default_occgrid_params with fields replaced"""
    return _params(OccGridParams, "ndtgpu_default_occgrid_params", "occupancy-grid", fields, hidden=("reserved_",))


def occupancy_grid_dims(res, cells_per_axis, centre, resolution):
    """ndtgpu_occgrid_dims: (width, height, origin[3]) of the occupancy grid of a map of cells_per_axis cells of `res` metres around
    `centre`, at pixel size `resolution`.  Plain numbers: needs no map set and no device."""
    cpa = (C.c_int32 * 3)(*[int(x) for x in cells_per_axis])
    c = _f64(centre).reshape(3)
    w, h = C.c_int32(), C.c_int32()
    origin = np.zeros(3)
    _check(lib().ndtgpu_occgrid_dims(float(res), cpa, _dp(c), float(resolution), C.byref(w), C.byref(h), _dp(origin)))
    return int(w.value), int(h.value), [float(x) for x in origin]


def occupancy_grid_move(T, origin_pose):
    """ndtgpu_occgrid_move (moveOccupancyMap): T * origin_pose, both 4 x 4"""
    a = np.ascontiguousarray(_f64(T).reshape(4, 4).T)                   # column-major
    b = np.ascontiguousarray(_f64(origin_pose).reshape(4, 4).T)
    m = np.zeros(16)
    lib().ndtgpu_occgrid_move(_dp(a), _dp(b), _dp(m))
    return m.reshape(4, 4).T.copy()


class LinkGateParams(C.Structure):
    _fields_ = [("max_score", C.c_double), ("max_dist", C.c_double), ("max_angle", C.c_double), ("min_idx_dist", C.c_int32),
                ("clip_cosine", C.c_int32)]


def linkgate_params(**fields):
    """ndtgpu_default_linkgate_params (0.1, 1.0, 0.2, 2, clip_cosine 0) with fields replaced"""
    return _params(LinkGateParams, "ndtgpu_default_linkgate_params", "link-gate", fields)


def _dev_ptr(t, dtype, numel, what):
    """the address of a contiguous torch device tensor of `dtype` with at least `numel` elements (None stays None)"""
    if t is None:
        return None
    if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.numel() >= numel):
        raise ValueError("%s: a contiguous device tensor of %s with at least %d elements is required" % (what, dtype, numel))
    return C.c_void_p(t.data_ptr())


class LinkGate(_Handle):
    """ndtgpu_linkgate: which links exist (include/ndtgpu.h "link gating") -- the candidate pairs of computeAllPossibleLinks gated
    by index distance and odometry, getValidLinks of the registered links, and the gather that packs what stays.  Works on torch
    device tensors; uint32 index arrays are int32 tensors (torch has no uint32 arithmetic; the bits are the same).  Poses are
    [n, 16] column-major on the device, [n, 4, 4] where a host array is taken."""
    _destroy = "ndtgpu_linkgate_destroy"

    def __init__(self, max_nodes, max_links):
        h = C.c_void_p()
        _check(lib().ndtgpu_linkgate_create(int(max_nodes), int(max_links), C.byref(h)))
        self.h, self.max_nodes, self.max_links, self.n_nodes = h, int(max_nodes), int(max_links), 0

    def set_nodes(self, T, stream=None):
        """the node poses: a host array [n, 4, 4] (synchronous), or a float64 device tensor [n, 16] column-major (on `stream`)"""
        if hasattr(T, "is_cuda"):
            n = T.numel() // 16
            import torch
            _check(lib().ndtgpu_linkgate_set_nodes_device(self.h, n, _dev_ptr(T, torch.float64, 16 * n, "LinkGate.set_nodes"), _stream_ptr(stream)))
        else:
            Tcm = np.ascontiguousarray(np.transpose(_f64(T).reshape(-1, 4, 4), (0, 2, 1)))
            n = Tcm.shape[0]
            _check(lib().ndtgpu_linkgate_set_nodes(self.h, n, _dp(Tcm) if n else None))
        self.n_nodes = n

    def candidates(self, capacity, with_T=True, stream=None, **params):
        """every pair i < j through the candidate gate: (ref int32 [capacity], mov int32 [capacity], T16 float64 [capacity, 16] or
        None) device tensors whose first count() entries are the survivors in computeAllPossibleLinks' order; asynchronous"""
        import torch
        cap = int(capacity)
        ref = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda")
        mov = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda")
        T16 = torch.empty((max(cap, 1), 16), dtype=torch.float64, device="cuda") if with_T else None
        self.candidates_into(ref, mov, T16, cap, stream=stream, **params)
        return ref, mov, T16

    def candidates_into(self, ref_dev, mov_dev, T16_dev, capacity, stream=None, **params):
        """candidates() into the caller's tensors (T16_dev may be None); nothing is written behind `capacity` entries"""
        import torch
        cap = int(capacity)
        p = linkgate_params(**params)
        _check(lib().ndtgpu_linkgate_candidates(self.h, C.byref(p), _dev_ptr(ref_dev, torch.int32, cap, "LinkGate.candidates ref"),
                                                _dev_ptr(mov_dev, torch.int32, cap, "LinkGate.candidates mov"),
                                                _dev_ptr(T16_dev, torch.float64, 16 * cap, "LinkGate.candidates T16"), cap, _stream_ptr(stream)))

    def valid(self, ref, mov, T16_dev, score_dev=None, keep_dev=None, capacity=None, stream=None, **params):
        """getValidLinks of the links (ref, mov, T16_dev [m, 16] column-major, score_dev [m] or None) under the set nodes.  ref / mov:
        int32 device tensors, or host arrays (uploaded, then the same entry).  The kept indices go to the handle's keep list and to
        keep_dev (int32 device tensor of `capacity` entries) where given; asynchronous"""
        import torch
        if not hasattr(ref, "is_cuda"):
            ref = torch.tensor(np.ascontiguousarray(ref, dtype=np.uint32).view(np.int32).reshape(-1), device="cuda")
            mov = torch.tensor(np.ascontiguousarray(mov, dtype=np.uint32).view(np.int32).reshape(-1), device="cuda")
        if not hasattr(T16_dev, "is_cuda"):
            Tcm = np.transpose(_f64(T16_dev).reshape(-1, 4, 4), (0, 2, 1))
            T16_dev = torch.tensor(np.ascontiguousarray(Tcm).reshape(Tcm.shape[0], 16), device="cuda")
        if score_dev is not None and not hasattr(score_dev, "is_cuda"):
            score_dev = torch.tensor(_f64(score_dev).reshape(-1), device="cuda")
        m = ref.numel()
        if mov.numel() != m:
            raise ValueError("LinkGate.valid: one ref and one mov index per link")
        cap = 0 if keep_dev is None else (keep_dev.numel() if capacity is None else int(capacity))
        p = linkgate_params(**params)
        self._inputs = (ref, mov, T16_dev, score_dev)       # (uploaded copies stay alive until the next call)
        _check(lib().ndtgpu_linkgate_valid(self.h, C.byref(p), m, _dev_ptr(ref, torch.int32, m, "LinkGate.valid ref"),
                                           _dev_ptr(mov, torch.int32, m, "LinkGate.valid mov"),
                                           _dev_ptr(T16_dev, torch.float64, 16 * m, "LinkGate.valid T16") if m else None,
                                           _dev_ptr(score_dev, torch.float64, m, "LinkGate.valid score"),
                                           _dev_ptr(keep_dev, torch.int32, cap, "LinkGate.valid keep"), cap, _stream_ptr(stream)))

    def gather(self, src_dev, dst_dev, dst_first_row=0, row_bytes=None, stream=None):
        """row keep[k] of src_dev -> row dst_first_row + k of dst_dev for the last valid() call's keep list; rows are the tensors'
        trailing dimensions (row_bytes: override); asynchronous, the count is read on the device"""
        if row_bytes is None:
            row_bytes = src_dev.element_size() * (src_dev.numel() // src_dev.shape[0] if src_dev.dim() > 1 else 1)
        if not (src_dev.is_cuda and dst_dev.is_cuda and src_dev.is_contiguous() and dst_dev.is_contiguous()):
            raise ValueError("LinkGate.gather: contiguous device tensors are required")
        _check(lib().ndtgpu_linkgate_gather(self.h, C.c_void_p(src_dev.data_ptr()), int(row_bytes), C.c_void_p(dst_dev.data_ptr()),
                                            int(dst_first_row), _stream_ptr(stream)))

    def count(self):
        """(count, overflow) of the last candidates() / valid() call; waits for the handle"""
        n, o = C.c_size_t(), C.c_int32()
        _check(lib().ndtgpu_linkgate_count(self.h, C.byref(n), C.byref(o)))
        return int(n.value), bool(o.value)

    def keep(self, first=0, n=None):
        """the last valid() call's keep list [first, first + n) as a host int64 array (n None: to the end, where valid() was the
        handle's last selection); waits for the handle"""
        if n is None:
            n = self.count()[0] - int(first)
        out = np.zeros(max(int(n), 1), dtype=np.uint32)
        _check(lib().ndtgpu_linkgate_keep(self.h, int(first), int(n), out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out[:int(n)].astype(np.int64)


def optimize_gated(pgo, g, gate, start_poses, incr_ref, incr_mov, incr_T16_dev, ref, mov, T16_dev, score_dev=None, cov36_dev=None,
                   cov_flags_dev=None, max_rounds=10, pgo_fields=None, wide=False, robust=None, **params):
    """The offline mapper's loop (ndt_feature_graph_opt.cpp:152-173) on the device: every round sets the gate's nodes to the current
    poses, runs getValidLinks (gate.valid) over the matched links (ref, mov host arrays; T16_dev [m, 16], score_dev [m], cov36_dev
    [m, 36], cov_flags_dev [m] device tensors), gathers T16 / cov36 / flags of the links that stay behind the incremental links
    (incr_ref, incr_mov host arrays, incr_T16_dev [k, 16]; their covariance is the flagged stand-in 0.02 I where cov36_dev is
    given), downloads ONLY the keep list, and optimises graph g of `pgo` from the current poses with incremental + kept links.
    It stops when the kept count repeats, when nothing is kept, or after max_rounds rounds -- max_rounds is OURS: upstream's loop
    has no cap and can oscillate between two link sets.  start_poses: [n, 3] (x, y, yaw).  **params: fields of
    ndtgpu_linkgate_params; pgo_fields: a dict of ndtgpu_pgo_params fields; wide: optimise with the chip-wide form
    (PGO.optimize_wide), the one for a large graph; robust: None -- the plain optimiser, call for call as before -- or a dict of
    ndtgpu_pgo_robust_params fields ({} for the defaults): every round optimises with PGO.optimize_robust instead, so a false
    closure the gate lets through is weighted down (PGO.robust_links(g) tells which, in the order incremental + kept of the last
    round).  Returns (kept index arrays per round, final poses [n, 3])."""
    import torch
    poses = _f64(start_poses).reshape(-1, 3).copy()
    n = poses.shape[0]
    iref = np.ascontiguousarray(incr_ref, dtype=np.uint32).reshape(-1)
    imov = np.ascontiguousarray(incr_mov, dtype=np.uint32).reshape(-1)
    ref = np.ascontiguousarray(ref, dtype=np.uint32).reshape(-1)
    mov = np.ascontiguousarray(mov, dtype=np.uint32).reshape(-1)
    k, m = iref.shape[0], ref.shape[0]
    ref_dev = torch.from_numpy(ref.view(np.int32)).cuda()
    mov_dev = torch.from_numpy(mov.view(np.int32)).cuda()
    T_all = torch.empty((k + m, 16), dtype=torch.float64, device="cuda")
    if k:
        T_all[:k] = incr_T16_dev.reshape(k, 16)
    cov_all = flags_all = None
    if cov36_dev is not None:
        cov_all = torch.zeros((k + m, 36), dtype=torch.float64, device="cuda")
        flags_all = torch.empty(k + m, dtype=torch.int32, device="cuda")
        flags_all[:k] = 4                                # NDTGPU_COV_NOT_COMPUTED: the factor takes 0.02 I for an incremental link
    rounds, prev = [], None
    for _ in range(int(max_rounds)):
        c, s = np.cos(poses[:, 2]), np.sin(poses[:, 2])
        T = np.tile(np.eye(4), (n, 1, 1))
        T[:, 0, 0], T[:, 0, 1], T[:, 1, 0], T[:, 1, 1], T[:, 0, 3], T[:, 1, 3] = c, -s, s, c, poses[:, 0], poses[:, 1]
        gate.set_nodes(T)
        gate.valid(ref_dev, mov_dev, T16_dev, score_dev, **params)
        gate.gather(T16_dev, T_all, dst_first_row=k, row_bytes=128)
        if cov_all is not None:
            gate.gather(cov36_dev, cov_all, dst_first_row=k, row_bytes=288)
            gate.gather(cov_flags_dev, flags_all, dst_first_row=k, row_bytes=4)
        kept = gate.keep()
        rounds.append(kept)
        if kept.size == 0:
            break
        torch.cuda.synchronize()                         # (the gathers ran on torch's stream; set_links_device takes complete arrays)
        pgo.set_links_device(g, poses, np.concatenate([iref, ref[kept]]), np.concatenate([imov, mov[kept]]), T_all, cov_all, flags_all)
        if robust is not None:
            pgo.optimize_robust(g, 1, robust=robust, wide=wide, **(pgo_fields or {}))
        elif wide:
            pgo.optimize_wide(g, **(pgo_fields or {}))
        else:
            pgo.optimize(g, 1, **(pgo_fields or {}))
        poses = pgo.poses(g)[0][:n].copy()
        if prev == kept.size:
            break
        prev = kept.size
    return rounds, poses


class FeatMatchParams(C.Structure):
    _fields_ = [("acceptance_threshold", C.c_double), ("success_probability", C.c_double), ("inlier_probability", C.c_double),
                ("distance_threshold", C.c_double), ("rigidity_threshold", C.c_double), ("seed", C.c_uint64), ("adaptive", C.c_int32),
                ("pad_", C.c_int32)]


class FeatMatchResult(C.Structure):
    _fields_ = [("score", C.c_double), ("x", C.c_double), ("y", C.c_double), ("theta", C.c_double), ("c", C.c_double), ("s", C.c_double),
                ("n_candidates", C.c_int32), ("n_hypotheses", C.c_int32), ("n_tested", C.c_int32), ("best_hypothesis", C.c_int32),
                ("n_inliers", C.c_int32), ("status", C.c_int32)]


FEATMATCH_RESULT_DTYPE = np.dtype([("score", "<f8"), ("x", "<f8"), ("y", "<f8"), ("theta", "<f8"), ("c", "<f8"), ("s", "<f8"),
                                   ("n_candidates", "<i4"), ("n_hypotheses", "<i4"), ("n_tested", "<i4"), ("best_hypothesis", "<i4"),
                                   ("n_inliers", "<i4"), ("status", "<i4")])
# ndtgpu_featmatch_result.status (include/ndtgpu.h NDTGPU_FEATMATCH_*)
FEATMATCH_OK, FEATMATCH_TOO_FEW, FEATMATCH_NO_HYPOTHESIS, FEATMATCH_BAD_INDEX = 0, 1, 2, 3


class FeatExtractParams(C.Structure):
    _fields_ = [("scales", C.c_int32), ("bin_rho", C.c_int32), ("bin_phi", C.c_int32), ("pad_", C.c_int32), ("base_sigma", C.c_double),
                ("sigma_step", C.c_double), ("dmst", C.c_double), ("min_value", C.c_double), ("min_diff", C.c_double),
                ("min_rho", C.c_double), ("max_rho", C.c_double), ("min_separation", C.c_double), ("r_min", C.c_double),
                ("r_max", C.c_double)]


class FeatExtractResult(C.Structure):
    _fields_ = [("n_valid", C.c_int32), ("n_segments", C.c_int32), ("n_peaks", C.c_int32), ("n_found", C.c_int32),
                ("n_stored", C.c_int32), ("status", C.c_int32)]


FEATEXTRACT_RESULT_DTYPE = np.dtype([("n_valid", "<i4"), ("n_segments", "<i4"), ("n_peaks", "<i4"), ("n_found", "<i4"),
                                     ("n_stored", "<i4"), ("status", "<i4")])
# ndtgpu_featextract_result.status (include/ndtgpu.h NDTGPU_FEATEXTRACT_*)
FEATEXTRACT_OK, FEATEXTRACT_TOO_FEW_POINTS, FEATEXTRACT_OVERFLOW, FEATEXTRACT_BAD_INDEX = 0, 1, 2, 3


def featextract_params(**fields):
    """ndtgpu_default_featextract_params with fields replaced"""
    return _params(FeatExtractParams, "ndtgpu_default_featextract_params", "feature-extraction", fields)


def featmatch_params(**fields):
    """ndtgpu_default_featmatch_params with fields replaced"""
    return _params(FeatMatchParams, "ndtgpu_default_featmatch_params", "feature-match", fields)


class FeatureMatcher(_Handle):
    """ndtgpu_featbank: n_sets feature sets of up to max_points points (position (x, y, theta) + descriptor of desc_len doubles) in
    device memory, and the RANSAC matching of pairs of them, one workgroup per pair (include/ndtgpu.h: matchFeatureMap)."""
    _destroy = "ndtgpu_featbank_destroy"

    def __init__(self, n_sets, max_points, desc_len=48):
        h = C.c_void_p()
        _check(lib().ndtgpu_featbank_create(int(n_sets), int(max_points), int(desc_len), C.byref(h)))
        self.h, self.n_sets, self.max_points, self.desc_len = h, int(n_sets), int(max_points), int(desc_len)

    def set(self, k, pos, desc):
        """set k: pos [n, 3] (x, y, theta), desc [n, desc_len]; n = 0 empties it"""
        ps = _f64(pos).reshape(-1, 3)
        ds = _f64(desc).reshape(-1, self.desc_len)
        if ps.shape[0] != ds.shape[0]:
            raise ValueError("FeatureMatcher.set: one descriptor per point")
        n = ps.shape[0]
        _check(lib().ndtgpu_featbank_set(self.h, int(k), n, _dp(ps) if n else None, _dp(ds) if n else None))

    def get(self, k):
        """set k as it stands in the bank -> (pos [n, 3], desc [n, desc_len] row-major); waits for the handle"""
        n = C.c_size_t()
        ps, ds = np.zeros((self.max_points, 3)), np.zeros((self.max_points, self.desc_len))
        _check(lib().ndtgpu_featbank_get(self.h, int(k), C.byref(n), _dp(ps), _dp(ds)))
        return ps[:n.value].copy(), ds[:n.value].copy()

    def extract(self, set_idx, ranges, angle_min, angle_increment, stream=None, **params):
        """laser scans ranges [n, n_beams] (beam i at angle_min + i * angle_increment) in one launch, scan b into set set_idx[b] ->
        (records [n] FEATEXTRACT_RESULT_DTYPE, list of n dicts(beam uint32 [n_stored], level int32, response float64)); keyword
        arguments: fields of ndtgpu_featextract_params"""
        si = np.ascontiguousarray(set_idx, dtype=np.uint32).reshape(-1)
        rr = np.ascontiguousarray(ranges, dtype=np.float64)
        n = si.shape[0]
        if rr.ndim != 2 or rr.shape[0] != n:
            raise ValueError("FeatureMatcher.extract: ranges must be [n_scans, n_beams], one row per set index")
        u32p = C.POINTER(C.c_uint32)
        p = featextract_params(**params)
        _check(lib().ndtgpu_featbank_extract(self.h, si.ctypes.data_as(u32p), _dp(rr), n, rr.shape[1], float(angle_min), float(angle_increment),
                                             C.byref(p), _stream_ptr(stream)))
        res = np.zeros(n, dtype=FEATEXTRACT_RESULT_DTYPE)
        beam = np.zeros((n, self.max_points), dtype=np.uint32)
        level = np.zeros((n, self.max_points), dtype=np.int32)
        resp = np.zeros((n, self.max_points))
        _check(lib().ndtgpu_featbank_extract_results(self.h, 0, n, C.c_void_p(res.ctypes.data), beam.ctypes.data_as(u32p),
                                                     level.ctypes.data_as(C.POINTER(C.c_int32)), _dp(resp)))
        return res, [dict(beam=beam[b, :res["n_stored"][b]].copy(), level=level[b, :res["n_stored"][b]].copy(),
                          response=resp[b, :res["n_stored"][b]].copy()) for b in range(n)]

    def extract_device(self, set_idx_dev, ranges_dev, angle_min, angle_increment, results_dev, beam_dev=None, level_dev=None,
                       response_dev=None, stream=None, **params):
        """the same on torch CUDA tensors, asynchronous on `stream`: set_idx_dev int32 [n] (read as uint32), ranges_dev float64
        [n, n_beams], results_dev uint8 [n * sizeof(ndtgpu_featextract_result)], beam_dev / level_dev int32 [n, max_points],
        response_dev float64 [n, max_points]"""
        n = int(set_idx_dev.numel())
        assert set_idx_dev.is_cuda and set_idx_dev.is_contiguous() and set_idx_dev.element_size() == 4
        assert ranges_dev.is_cuda and ranges_dev.is_contiguous() and ranges_dev.element_size() == 8 and ranges_dev.dim() == 2
        assert ranges_dev.shape[0] == n
        assert results_dev.is_cuda and results_dev.is_contiguous() and results_dev.numel() * results_dev.element_size() >= n * C.sizeof(FeatExtractResult)
        for t, size in ((beam_dev, 4), (level_dev, 4), (response_dev, 8)):
            if t is not None:
                assert t.is_cuda and t.is_contiguous() and t.element_size() == size and t.numel() >= n * self.max_points
        p = featextract_params(**params)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _check(lib().ndtgpu_featbank_extract_device(self.h, ptr(set_idx_dev), ptr(ranges_dev), n, int(ranges_dev.shape[1]), float(angle_min),
                                                    float(angle_increment), C.byref(p), ptr(results_dev), ptr(beam_dev), ptr(level_dev),
                                                    ptr(response_dev), _stream_ptr(stream)))

    def match(self, ref_idx, mov_idx, stream=None, **params):
        """pairs (ref_idx[p], mov_idx[p]) in one launch -> (results [n] FEATMATCH_RESULT_DTYPE, T [n, 4, 4] mov -> ref, list of n
        correspondence arrays [n_inliers, 2] uint32 (mov_i, ref_j)); keyword arguments: fields of ndtgpu_featmatch_params"""
        ri = np.ascontiguousarray(ref_idx, dtype=np.uint32).reshape(-1)
        mi = np.ascontiguousarray(mov_idx, dtype=np.uint32).reshape(-1)
        if ri.shape != mi.shape:
            raise ValueError("FeatureMatcher.match: one ref and one mov index per pair")
        n = ri.shape[0]
        u32p = C.POINTER(C.c_uint32)
        p = featmatch_params(**params)
        _check(lib().ndtgpu_featbank_match(self.h, ri.ctypes.data_as(u32p), mi.ctypes.data_as(u32p), n, C.byref(p), _stream_ptr(stream)))
        res = np.zeros(n, dtype=FEATMATCH_RESULT_DTYPE)
        T = np.zeros((n, 16))
        corr = np.zeros((n, self.max_points, 2), dtype=np.uint32)
        _check(lib().ndtgpu_featbank_results(self.h, 0, n, C.c_void_p(res.ctypes.data), _dp(T), corr.ctypes.data_as(u32p)))
        return res, np.transpose(T.reshape(n, 4, 4), (0, 2, 1)).copy(), [corr[k, :res["n_inliers"][k]].copy() for k in range(n)]

    def match_device(self, ref_idx_dev, mov_idx_dev, results_dev, T16_dev=None, corr_dev=None, stream=None, **params):
        """the same on torch CUDA tensors, asynchronous on `stream`: ref_idx_dev / mov_idx_dev int32 [n] (read as uint32),
        results_dev uint8 [n * sizeof(ndtgpu_featmatch_result)], T16_dev float64 [n, 16] (column-major, ready for
        match_batch_device), corr_dev int32 [n, max_points, 2]"""
        n = int(ref_idx_dev.numel())
        assert ref_idx_dev.is_cuda and mov_idx_dev.is_cuda and ref_idx_dev.element_size() == 4 and mov_idx_dev.element_size() == 4
        assert mov_idx_dev.numel() == n and ref_idx_dev.is_contiguous() and mov_idx_dev.is_contiguous()
        assert results_dev.is_cuda and results_dev.is_contiguous() and results_dev.numel() * results_dev.element_size() >= n * C.sizeof(FeatMatchResult)
        if T16_dev is not None:
            assert T16_dev.is_cuda and T16_dev.is_contiguous() and T16_dev.element_size() == 8 and T16_dev.numel() >= 16 * n
        if corr_dev is not None:
            assert corr_dev.is_cuda and corr_dev.is_contiguous() and corr_dev.element_size() == 4 and corr_dev.numel() >= 2 * n * self.max_points
        p = featmatch_params(**params)
        _check(lib().ndtgpu_featbank_match_device(self.h, C.c_void_p(ref_idx_dev.data_ptr()), C.c_void_p(mov_idx_dev.data_ptr()), n, C.byref(p),
                                                  C.c_void_p(results_dev.data_ptr()), None if T16_dev is None else C.c_void_p(T16_dev.data_ptr()),
                                                  None if corr_dev is None else C.c_void_p(corr_dev.data_ptr()), _stream_ptr(stream)))


class FuserParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("map_size_x", C.c_double), ("map_size_y", C.c_double), ("map_size_z", C.c_double),
                ("sensor_range", C.c_double), ("max_translation_norm", C.c_double), ("max_rotation_norm", C.c_double),
                ("check_consistency", C.c_int32), ("fuse_incomplete", C.c_int32), ("use_odom", C.c_int32), ("neighbours", C.c_int32),
                ("stepcontrol", C.c_int32), ("itr_max", C.c_int32), ("delta_score", C.c_double), ("force_odom_as_est", C.c_int32),
                ("fusion2d", C.c_int32), ("all_matches_valid", C.c_int32), ("use_soft_constraints", C.c_int32), ("compute_cov", C.c_int32),
                ("step_control_fusion", C.c_int32), ("use_tikhonov", C.c_int32), ("covariance_mode", C.c_int32),
                ("discard_cells", C.c_int32), ("pad_", C.c_int32),
                ("motion_Cd", C.c_double), ("motion_Ct", C.c_double), ("motion_Dd", C.c_double), ("motion_Dt", C.c_double),
                ("motion_Td", C.c_double), ("motion_Tt", C.c_double), ("sensor_pose", C.c_double * 16), ("max_cells", C.c_uint32)]


class FuserPrepared(C.Structure):
    _fields_ = [("Tscan", C.c_double * 16), ("scan_centre", C.c_double * 3), ("range_origin", C.c_double * 3), ("Tcov", C.c_double * 36),
                ("odom_cov", C.c_double * 9), ("feat_src_mean", C.c_double * 3), ("feat_tgt_mean", C.c_double * 3),
                ("feat_cov_rotated", C.c_double * 6), ("feat_cov_plain", C.c_double * 6)]


FUSER_RESULT_DTYPE = np.dtype([("Tnow", "<f8", (16,)), ("Tmotion_est", "<f8", (16,)), ("spose", "<f8", (16,)), ("match", RESULT_DTYPE),
                               ("match_ok", "<i4"), ("registration_failure", "<i4"), ("cov_singular", "<i4"), ("pad_", "<i4"),
                               ("posecov_mean", "<f8", (3,)), ("posecov", "<f8", (9,))])


class FuserFeatParams(C.Structure):
    _fields_ = [("use_feat", C.c_int32), ("prev_in_map_frame", C.c_int32), ("map_every", C.c_int32), ("pad_", C.c_int32),
                ("feat_cov", C.c_double * 3), ("match", FeatMatchParams)]


class FuserFeatResult(C.Structure):
    _fields_ = [("ransac", FeatMatchResult), ("Tfeat", C.c_double * 16), ("ransac_run", C.c_int32), ("consistent", C.c_int32),
                ("n_feat_cells", C.c_int32), ("n_odom_cells", C.c_int32), ("truncated", C.c_int32), ("n_prev", C.c_int32),
                ("n_map", C.c_int32), ("map_appended", C.c_int32), ("map_overflow", C.c_int32), ("pad_", C.c_int32)]


FUSER_FEAT_RESULT_DTYPE = np.dtype([("ransac", FEATMATCH_RESULT_DTYPE), ("Tfeat", "<f8", (16,)), ("ransac_run", "<i4"), ("consistent", "<i4"),
                                    ("n_feat_cells", "<i4"), ("n_odom_cells", "<i4"), ("truncated", "<i4"), ("n_prev", "<i4"),
                                    ("n_map", "<i4"), ("map_appended", "<i4"), ("map_overflow", "<i4"), ("pad_", "<i4")])
assert FUSER_FEAT_RESULT_DTYPE.itemsize == C.sizeof(FuserFeatResult)


def fuser_feat_params(**fields):
    """ndtgpu_default_fuser_feat_params with fields replaced; feat_cov: 3 numbers; match: a FeatMatchParams or a dict of its fields"""
    p = FuserFeatParams()
    lib().ndtgpu_default_fuser_feat_params(C.byref(p))
    for k, v in fields.items():
        if k == "feat_cov":
            p.feat_cov[:] = [float(x) for x in v]
        elif k == "match":
            p.match = v if isinstance(v, FeatMatchParams) else featmatch_params(**v)
        elif k not in dict(FuserFeatParams._fields_):
            raise TypeError("fuser_feat_params: no field %r" % k)
        else:
            setattr(p, k, v)
    return p


def fuser_feat_prepare(params, feat_params, Tnow, Tmotion, ransac, corr, cur_pos, prev_pos, prev_moved=False):
    """ndtgpu_fuser_feat_prepare: the gate and the cell records of one slot, no device.  Tnow / Tmotion: 4x4 row-major NumPy;
    ransac: a FEATMATCH_RESULT_DTYPE record (or None: RANSAC not run); corr [n_inliers, 2] (cur i, prev j); cur_pos / prev_pos [n, 3]
    -> (record FUSER_FEAT_RESULT_DTYPE [1], cells [n_cells, 18])"""
    tn = np.ascontiguousarray(np.asarray(Tnow, dtype=np.float64).T).reshape(16).copy()
    tm = np.ascontiguousarray(np.asarray(Tmotion, dtype=np.float64).T).reshape(16).copy()
    cp, pp = _f64(cur_pos).reshape(-1, 3), _f64(prev_pos).reshape(-1, 3)
    rec = np.zeros(1, dtype=FUSER_FEAT_RESULT_DTYPE)
    cells = np.zeros((64, 18))
    n = C.c_uint32()
    rp = None
    if ransac is not None:
        rr = np.zeros(1, dtype=FEATMATCH_RESULT_DTYPE)
        rr[0] = ransac
        rp = C.cast(C.c_void_p(rr.ctypes.data), C.POINTER(FeatMatchResult))
    cr = np.ascontiguousarray(corr if corr is not None else np.zeros((0, 2)), dtype=np.uint32).reshape(-1, 2)
    u32p = C.POINTER(C.c_uint32)
    _check(lib().ndtgpu_fuser_feat_prepare(C.byref(params), C.byref(feat_params), _dp(tn), _dp(tm), rp, cr.ctypes.data_as(u32p) if cr.size else None,
                                           _dp(cp) if cp.size else None, cp.shape[0], _dp(pp) if pp.size else None, pp.shape[0],
                                           1 if prev_moved else 0, C.cast(C.c_void_p(rec.ctypes.data), C.POINTER(FuserFeatResult)), _dp(cells),
                                           C.byref(n)))
    return rec, cells[:n.value].copy()


def fuser_feat_move(T, pos):
    """ndtgpu_fuser_feat_move: points [n, 3] (x, y, theta) moved by the 4x4 row-major T (moveInterestPointVec)"""
    t = np.ascontiguousarray(np.asarray(T, dtype=np.float64).T).reshape(16).copy()
    ps = _f64(pos).reshape(-1, 3)
    out = np.zeros_like(ps)
    _check(lib().ndtgpu_fuser_feat_move(_dp(t), _dp(ps) if ps.size else None, ps.shape[0], _dp(out) if ps.size else None))
    return out


def fuser_params(**fields):
    """ndtgpu_default_fuser_params with fields overridden; sensor_pose: 4x4 (row-major NumPy) or 16 column-major numbers."""
    p = FuserParams()
    lib().ndtgpu_default_fuser_params(C.byref(p))
    for k, v in fields.items():
        if k == "sensor_pose":
            a = np.asarray(v, dtype=np.float64)
            p.sensor_pose[:] = list(a.T.reshape(16) if a.shape == (4, 4) else a.reshape(16))
        elif k not in dict(FuserParams._fields_):
            raise TypeError("fuser_params: no field %r" % k)
        else:
            setattr(p, k, v)
    return p


def fuser_prepare(params, Tnow, Tmotion, node_centre):
    """ndtgpu_fuser_prepare: what the host derives from (pose, odometry increment).  Tnow / Tmotion: 4x4 row-major NumPy."""
    out = FuserPrepared()
    tn = np.ascontiguousarray(np.asarray(Tnow, dtype=np.float64).T).reshape(16).copy()
    tm = np.ascontiguousarray(np.asarray(Tmotion, dtype=np.float64).T).reshape(16).copy()
    nc = _f64(node_centre).reshape(3)
    _check(lib().ndtgpu_fuser_prepare(C.byref(params), _dp(tn), _dp(tm), _dp(nc), C.byref(out)))
    return {k: np.array(getattr(out, k)) for k, _ in FuserPrepared._fields_}


class FuserBank(_Handle):
    """ndtgpu_fuser_bank: NDTFeatureFuserHMT::initialize / update for a batch of independent fusers, one asynchronous call
    each (include/ndtgpu.h).  Poses are 4x4 row-major NumPy arrays on this side."""
    _destroy = "ndtgpu_fuser_bank_destroy"

    def __init__(self, params, n_fusers, node_maps=None):
        h = C.c_void_p()
        _check(lib().ndtgpu_fuser_bank_create(C.byref(params), int(n_fusers), node_maps.h if node_maps is not None else None, C.byref(h)))
        self.h, self.n, self.params = h, int(n_fusers), params
        self._node_maps = node_maps       # (kept alive)

    def mapsets(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(lib().ndtgpu_fuser_bank_mapsets(self.h, C.byref(a), C.byref(b)))
        return _BorrowedMapSet(a, self.n, self.params.resolution), _BorrowedMapSet(b, self.n, self.params.resolution)

    @staticmethod
    def _poses16(T, n):
        return np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).reshape(n, 16).copy()

    def _cloud_args(self, xyz):
        import torch
        assert xyz.dtype == torch.float32 and xyz.is_cuda and xyz.stride(2) == 1 and xyz.stride(1) == xyz.shape[2]
        return C.c_void_p(xyz.data_ptr()), int(xyz.shape[1]), 4 * int(xyz.shape[2]), 4 * int(xyz.stride(0))

    def attach_features(self, fm, prev_first, map_first, **params):
        """ndtgpu_fuser_bank_attach_features: fm a FeatureMatcher (kept alive); slot k's prev / map sets are prev_first + k /
        map_first + k; keyword arguments: fields of ndtgpu_fuser_feat_params (fuser_feat_params)"""
        p = fuser_feat_params(**params)
        _check(lib().ndtgpu_fuser_bank_attach_features(self.h, fm.h, int(prev_first), int(map_first), C.byref(p)))
        self._features, self.feat_params = fm, p

    @staticmethod
    def _sets(cur_sets, n):
        si = np.ascontiguousarray(cur_sets, dtype=np.uint32).reshape(-1)
        if si.shape[0] != n:
            raise ValueError("FuserBank: one cur set index per cloud")
        return si

    def initialize(self, init_poses, xyz, first=0, stream=None, cur_sets=None):
        """cur_sets: the feature-bank sets that hold the scans' interest points (the feature path); None: the plain entry"""
        n = int(xyz.shape[0])
        T = self._poses16(init_poses, n)
        ptr, npts, stride, mstride = self._cloud_args(xyz)
        if cur_sets is None:
            _check(lib().ndtgpu_fuser_initialize_batch(self.h, int(first), n, _dp(T), ptr, npts, stride, mstride, _stream_ptr(stream)))
            return
        si = self._sets(cur_sets, n)
        _check(lib().ndtgpu_fuser_initialize_batch_feat(self.h, int(first), n, _dp(T), ptr, npts, stride, mstride,
                                                        si.ctypes.data_as(C.POINTER(C.c_uint32)), _stream_ptr(stream)))

    def update(self, Tmotion, xyz, first=0, update_ndt_map=True, stream=None, cur_sets=None, update_feature_map=True):
        """cur_sets / update_feature_map: the feature path (ndtgpu_fuser_update_batch_feat); cur_sets None: the plain entry"""
        n = int(xyz.shape[0])
        T = self._poses16(Tmotion, n)
        ptr, npts, stride, mstride = self._cloud_args(xyz)
        if cur_sets is None:
            _check(lib().ndtgpu_fuser_update_batch(self.h, int(first), n, _dp(T), ptr, npts, stride, mstride, 1 if update_ndt_map else 0,
                                                   _stream_ptr(stream)))
            return
        si = self._sets(cur_sets, n)
        _check(lib().ndtgpu_fuser_update_batch_feat(self.h, int(first), n, _dp(T), ptr, npts, stride, mstride,
                                                    si.ctypes.data_as(C.POINTER(C.c_uint32)), 1 if update_feature_map else 0,
                                                    1 if update_ndt_map else 0, _stream_ptr(stream)))

    def feat_results(self, first=0, count=None):
        """the feature records of the last call with cur_sets: FUSER_FEAT_RESULT_DTYPE [n]; waits for the bank"""
        n = self.n - first if count is None else int(count)
        res = np.zeros(n, dtype=FUSER_FEAT_RESULT_DTYPE)
        _check(lib().ndtgpu_fuser_feat_results(self.h, int(first), n, C.c_void_p(res.ctypes.data)))
        return res

    def feat_cells(self, first=0, count=None):
        """the cell records the last update handed to the matcher -> list of n arrays [n_cells, 18]; waits for the bank"""
        n = self.n - first if count is None else int(count)
        off = np.zeros(n + 1, dtype=np.uint32)
        cells = np.zeros((64 * max(n, 1), 18))
        _check(lib().ndtgpu_fuser_feat_cells(self.h, int(first), n, off.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(cells), cells.shape[0]))
        return [cells[off[k]:off[k + 1]].copy() for k in range(n)]

    def poses(self, first=0, count=None):
        """-> (Tnow [n,4,4] row-major, results of the last update call: FUSER_RESULT_DTYPE [n]); waits for the bank"""
        n = self.n - first if count is None else int(count)
        T = np.zeros((n, 16))
        res = np.zeros(n, dtype=FUSER_RESULT_DTYPE)
        _check(lib().ndtgpu_fuser_poses(self.h, int(first), n, _dp(T), C.c_void_p(res.ctypes.data)))
        return np.transpose(T.reshape(n, 4, 4), (0, 2, 1)).copy(), res


class ScanProjectParams(C.Structure):
    _fields_ = [("r_min", C.c_double), ("r_max", C.c_double), ("varz", C.c_double), ("seed", C.c_uint64)]


SCANPROJECT_TILE = 1024      # ndtgpu_scanproj_tile(): the beams of a tile


def scanproject_params(**fields):
    """ndtgpu_default_scanproject_params (r_min 0.5, r_max 30.0, varz 0.02, seed 0) with fields replaced"""
    return _params(ScanProjectParams, "ndtgpu_default_scanproject_params", "scan-projection", fields)


def scan_project_beam(angle_min, angle_increment, scan_id, i, r, **params):
    """ndtgpu_scanproj_beam on the host: (x, y, z) as float32 [3] of beam i with range r of scan scan_id, or None where the beam
    is dropped"""
    p = scanproject_params(**params)
    xyz = (C.c_float * 3)()
    kept = lib().ndtgpu_scanproj_beam(C.byref(p), float(angle_min), float(angle_increment), int(scan_id), int(i), float(r), xyz)
    return np.array(xyz[:], dtype=np.float32) if kept else None


class ScanProjector(_Handle):
    """ndtgpu_scanproj: a batch of laser scans (ranges, beam i at angle_min + i * angle_increment) to the clouds in the sensor frame
    that the fuser bank and the registrar take (include/ndtgpu.h "laser-scan projection"): the kept points in beam order, NaN rows
    behind them."""
    _destroy = "ndtgpu_scanproj_destroy"

    def __init__(self, max_scans, max_beams):
        h = C.c_void_p()
        _check(lib().ndtgpu_scanproj_create(int(max_scans), int(max_beams), C.byref(h)))
        self.h, self.max_scans, self.max_beams = h, int(max_scans), int(max_beams)

    def project(self, ranges, angle_min, angle_increment, scan_ids=None, stride=12, **params):
        """HOST ranges [n, n_beams] -> (xyz float32 [n, n_beams, stride / 4] -- floats behind the fourth are zero --, n_kept uint32
        [n]); scan_ids: n ids (None: 0 .. n - 1); keyword arguments: fields of ndtgpu_scanproject_params.  Synchronous."""
        rr = np.ascontiguousarray(ranges, dtype=np.float64)
        if rr.ndim != 2 or stride % 4 != 0:
            raise ValueError("ScanProjector.project: ranges must be [n_scans, n_beams] and stride a multiple of 4")
        n, nb = rr.shape
        ids = None if scan_ids is None else np.ascontiguousarray(scan_ids, dtype=np.uint64).reshape(-1)
        if ids is not None and ids.shape[0] != n:
            raise ValueError("ScanProjector.project: one scan id per scan")
        xyz = np.zeros((n, nb, stride // 4), dtype=np.float32)
        kept = np.zeros(n, dtype=np.uint32)
        p = scanproject_params(**params)
        _check(lib().ndtgpu_scanproj_project(self.h, _dp(rr), None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint64)), n, nb,
                                             float(angle_min), float(angle_increment), C.byref(p), C.c_void_p(xyz.ctypes.data), int(stride),
                                             nb * int(stride), kept.ctypes.data_as(C.POINTER(C.c_uint32))))
        return xyz, kept

    def project_device(self, ranges_t, xyz_t, angle_min, angle_increment, scan_ids_t=None, n_kept_t=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream`: ranges_t float64 [n, n_beams] contiguous; xyz_t float32
        [n, n_beams, w >= 3], possibly a view of a larger tensor -- its strides give stride_bytes (rows) and map_stride_bytes
        (scans), and a row stride of 4 floats or more gets the fourth float written; scan_ids_t int64 / uint64 [n] (None: 0 .. n - 1);
        n_kept_t int32 [n] (read as uint32; may be None)"""
        import torch
        if not (ranges_t.is_cuda and ranges_t.is_contiguous() and ranges_t.dtype == torch.float64 and ranges_t.dim() == 2):
            raise ValueError("ScanProjector.project_device: ranges_t must be a contiguous float64 device tensor [n_scans, n_beams]")
        n, nb = int(ranges_t.shape[0]), int(ranges_t.shape[1])
        if not (xyz_t.is_cuda and xyz_t.dtype == torch.float32 and xyz_t.dim() == 3 and xyz_t.shape[0] == n and xyz_t.shape[1] == nb and
                xyz_t.shape[2] >= 3 and (xyz_t.stride(2) == 1)):
            raise ValueError("ScanProjector.project_device: xyz_t must be a float32 device tensor [n_scans, n_beams, >= 3] with unit "
                             "stride along its last axis")
        if scan_ids_t is not None and not (scan_ids_t.is_cuda and scan_ids_t.is_contiguous() and scan_ids_t.element_size() == 8 and
                                           scan_ids_t.numel() == n):
            raise ValueError("ScanProjector.project_device: scan_ids_t must be a contiguous 64-bit integer device tensor [n_scans]")
        p = scanproject_params(**params)
        _check(lib().ndtgpu_scanproj_project_device(self.h, C.c_void_p(ranges_t.data_ptr()),
                                                    None if scan_ids_t is None else C.c_void_p(scan_ids_t.data_ptr()), n, nb,
                                                    float(angle_min), float(angle_increment), C.byref(p), C.c_void_p(xyz_t.data_ptr()),
                                                    4 * int(xyz_t.stride(1)), 4 * int(xyz_t.stride(0)) if n > 1 else 4 * nb * int(xyz_t.stride(1)),
                                                    _dev_ptr(n_kept_t, torch.int32, n, "ScanProjector.project_device n_kept_t"),
                                                    _stream_ptr(stream)))


CALIB_TILE = 256             # ndtgpu_calib_tile(): the candidates of a workgroup
CALIB_NO_RESULT, CALIB_BAD_PAIR = 1, 2


def calib_params(**fields):
    """ndtgpu_default_calib_params (max_dist 0.1) with fields replaced"""
    return _params(CalibParams, "ndtgpu_default_calib_params", "calibration", fields)


def calib_lattice(ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r):
    """ndtgpu_calib_lattice: the candidates of bruteForceOptimization -> dict(xs [nx], ys [ny], yaws [nyaw], cs, sn [nyaw])"""
    a = [float(v) for v in (ix, iy, iyaw, x_s, y_s, yaw_s, t_r, yaw_r)]
    cnt = (C.c_size_t * 3)()
    _check(lib().ndtgpu_calib_lattice(*a, cnt, None, None, None, None, None, 0))
    room = max(cnt[:])
    xs, ys, yaws, cs, sn = (np.zeros(room) for _ in range(5))
    _check(lib().ndtgpu_calib_lattice(*a, cnt, _dp(xs), _dp(ys), _dp(yaws), _dp(cs), _dp(sn), room))
    nx, ny, nyaw = cnt[:]
    return dict(xs=xs[:nx].copy(), ys=ys[:ny].copy(), yaws=yaws[:nyaw].copy(), cs=cs[:nyaw].copy(), sn=sn[:nyaw].copy())


def calib_pair_motion(pose1, pose2):
    """ndtgpu_calib_pair_motion: D = pose1^-1 pose2 as (dx, dy, cd, sd) of two poses (x, y, c, s)"""
    p1, p2, D = _f64(pose1).reshape(4), _f64(pose2).reshape(4), np.zeros(4)
    _check(lib().ndtgpu_calib_pair_motion(_dp(p1), _dp(p2), _dp(D)))
    return D


def calib_select_pairs(poses4, max_translation=1.0, min_yaw=25.0 * np.pi / 180.0):
    """ndtgpu_calib_select_pairs: the callback's anchor and gate walk over poses (x, y, c, s) [n, 4] -> pairs uint32 [m, 2]"""
    pp = _f64(poses4).reshape(-1, 4)
    n = pp.shape[0]
    pairs = np.zeros((max(n, 1), 2), dtype=np.uint32)
    m = C.c_size_t()
    _check(lib().ndtgpu_calib_select_pairs(_dp(pp), n, float(max_translation), float(min_yaw), pairs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           pairs.shape[0], C.byref(m)))
    return pairs[:m.value].copy()


def _lattice_tables(lattice, who):
    """the tables xs, ys, cs, sn of a lattice (what calib_lattice returns) as flat float64 arrays"""
    t = [_f64(lattice[k]).reshape(-1) for k in ("xs", "ys", "cs", "sn")]
    if t[2].shape != t[3].shape:
        raise ValueError("%s: cs and sn must have one entry per yaw" % who)
    return t


class Calibrator(_Handle):
    """ndtgpu_calib: the laser's pose on the base by brute-force search over sensor offsets (include/ndtgpu.h "extrinsic
    calibration").  Clouds are a bank in the layout ScanProjector writes; poses are (x, y, cos yaw, sin yaw) of the base; pairs are
    (scan of cloud1, scan of cloud2); the lattice is what calib_lattice returns."""
    _destroy = "ndtgpu_calib_destroy"

    def __init__(self, max_pairs, max_points, max_candidates):
        h = C.c_void_p()
        _check(lib().ndtgpu_calib_create(int(max_pairs), int(max_points), int(max_candidates), C.byref(h)))
        self.h = h

    def search(self, xyz, n_kept, poses4, pairs, lattice, want_volume=False, **params):
        """HOST xyz float32 [n_scans, n_points, w >= 3], n_kept [n_scans], poses4 [n_scans, 4], pairs [n_pairs, 2] ->
        dict(index, ix, iy, iyaw, score, flags, n_skipped, volume [nx, ny, nyaw] or None).  Synchronous."""
        pts = np.ascontiguousarray(xyz, dtype=np.float32)
        if pts.ndim != 3 or pts.shape[2] < 3:
            raise ValueError("Calibrator.search: xyz must be [n_scans, n_points, >= 3]")
        n, npts, w = pts.shape
        kept = np.ascontiguousarray(n_kept, dtype=np.uint32).reshape(-1)
        pp = _f64(poses4).reshape(-1, 4)
        pr = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        if kept.shape[0] != n or pp.shape[0] != n:
            raise ValueError("Calibrator.search: one n_kept and one pose per scan")
        xs, ys, cs, sn = _lattice_tables(lattice, "Calibrator")
        vol = np.zeros(xs.shape[0] * ys.shape[0] * cs.shape[0]) if want_volume else None
        res = CalibResult()
        p = calib_params(**params)
        u32 = C.POINTER(C.c_uint32)
        _check(lib().ndtgpu_calib_search(self.h, C.c_void_p(pts.ctypes.data), n, npts, 4 * w, 4 * w * npts, kept.ctypes.data_as(u32), _dp(pp),
                                         pr.ctypes.data_as(u32), pr.shape[0], _dp(xs), xs.shape[0], _dp(ys), ys.shape[0], _dp(cs), _dp(sn),
                                         cs.shape[0], C.byref(p), C.byref(res), None if vol is None else _dp(vol)))
        return self._result(res.score, res.index, res.flags, res.n_skipped, vol, xs.shape[0], ys.shape[0], cs.shape[0])

    @staticmethod
    def _result(score, index, flags, n_skipped, vol, nx, ny, nyaw):
        index = int(index)
        return dict(index=index, ix=index // (ny * nyaw), iy=(index // nyaw) % ny, iyaw=index % nyaw, score=float(score), flags=int(flags),
                    n_skipped=int(n_skipped), volume=None if vol is None else vol.reshape(nx, ny, nyaw))

    def search_device(self, xyz_t, n_kept_t, poses_t, pairs_t, lattice, result_t, volume_t=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream`: xyz_t float32 [n_scans, n_points, w >= 3], possibly a view (its
        strides give stride_bytes and map_stride_bytes); n_kept_t int32 [n_scans] (read as uint32); poses_t float64 [n_scans, 4];
        pairs_t int32 [n_pairs, 2]; result_t: 24 bytes of device memory (CALIB_RESULT_DTYPE; a uint8 [24] or int32 [6] tensor);
        volume_t float64 [nx * ny * nyaw] or None.  read_result(result_t) decodes the record once the stream has run."""
        import torch
        if not (xyz_t.is_cuda and xyz_t.dtype == torch.float32 and xyz_t.dim() == 3 and xyz_t.shape[2] >= 3 and xyz_t.stride(2) == 1):
            raise ValueError("Calibrator.search_device: xyz_t must be a float32 device tensor [n_scans, n_points, >= 3] with unit stride "
                             "along its last axis")
        n, npts = int(xyz_t.shape[0]), int(xyz_t.shape[1])
        if not (pairs_t.is_cuda and pairs_t.is_contiguous() and pairs_t.dtype == torch.int32 and pairs_t.dim() == 2 and pairs_t.shape[1] == 2):
            raise ValueError("Calibrator.search_device: pairs_t must be a contiguous int32 device tensor [n_pairs, 2]")
        if not (result_t.is_cuda and result_t.is_contiguous() and result_t.numel() * result_t.element_size() >= 24):
            raise ValueError("Calibrator.search_device: result_t must be a contiguous device tensor of at least 24 bytes")
        xs, ys, cs, sn = _lattice_tables(lattice, "Calibrator")
        nc = xs.shape[0] * ys.shape[0] * cs.shape[0]
        p = calib_params(**params)
        _check(lib().ndtgpu_calib_search_device(self.h, C.c_void_p(xyz_t.data_ptr()), n, npts, 4 * int(xyz_t.stride(1)),
                                                4 * int(xyz_t.stride(0)) if n > 1 else 4 * npts * int(xyz_t.stride(1)),
                                                _dev_ptr(n_kept_t, torch.int32, n, "Calibrator.search_device n_kept_t"),
                                                _dev_ptr(poses_t, torch.float64, 4 * n, "Calibrator.search_device poses_t"),
                                                C.c_void_p(pairs_t.data_ptr()), int(pairs_t.shape[0]), _dp(xs), xs.shape[0], _dp(ys), ys.shape[0],
                                                _dp(cs), _dp(sn), cs.shape[0], C.byref(p), C.c_void_p(result_t.data_ptr()),
                                                _dev_ptr(volume_t, torch.float64, nc, "Calibrator.search_device volume_t"), _stream_ptr(stream)))

    @staticmethod
    def read_result(result_t):
        """the record search_device wrote (synchronises through the copy to the host): CALIB_RESULT_DTYPE scalar"""
        import torch
        return np.frombuffer(result_t.view(torch.uint8).cpu().numpy().tobytes()[:24], dtype=CALIB_RESULT_DTYPE)[0]


LOCMON_TILE = 256            # ndtgpu_locmon_tile()
LOCMON_NO_BEAMS, LOCMON_BAD_INDEX, LOCMON_NO_QUERY, LOCMON_NO_RESULT, LOCMON_NO_PICK = 1, 2, 4, 8, 16
LOCMON_KEY_FAR, LOCMON_KEY_OFFMAP, LOCMON_NO_SCAN = 0x10000, 0x10001, 0xFFFFFFFF


def locmon_params(**fields):
    """ndtgpu_default_locmon_params (max_dist 0.375, r_min 0, r_max inf, post (-0.275, 0), occupied_min 55, min_num_matches 8) with
    fields replaced"""
    return _params(LocmonParams, "ndtgpu_default_locmon_params", "localisation-monitor", fields)


def locmon_radius(max_dist, resolution):
    """ndtgpu_locmon_radius: R = (int)floor(max_dist / resolution), 1 .. 254"""
    R = C.c_int32()
    _check(lib().ndtgpu_locmon_radius(float(max_dist), float(resolution), C.byref(R)))
    return R.value


def locmon_beam_table(n_beams, angle_min, angle_increment):
    """ndtgpu_locmon_beam_table -> (cb [n_beams], sb [n_beams])"""
    cb, sb = np.zeros(int(n_beams)), np.zeros(int(n_beams))
    _check(lib().ndtgpu_locmon_beam_table(int(n_beams), float(angle_min), float(angle_increment), _dp(cb), _dp(sb)))
    return cb, sb


def locmon_pixel(pose4, cb, sb, r, origin2, resolution, width, height):
    """ndtgpu_locmon_pixel -> (fi, fj), or None where the endpoint is off the map"""
    p, o = _f64(pose4).reshape(4), _f64(origin2).reshape(2)
    cell, inb = (C.c_int32 * 2)(), C.c_int32()
    _check(lib().ndtgpu_locmon_pixel(_dp(p), float(cb), float(sb), float(r), _dp(o), float(resolution), int(width), int(height), cell,
                                     C.byref(inb)))
    return (cell[0], cell[1]) if inb.value else None


def locmon_metres(key, resolution, max_dist):
    """ndtgpu_locmon_metres: the badness of a key"""
    out = np.zeros(1)
    _check(lib().ndtgpu_locmon_metres(int(key), float(resolution), float(max_dist), _dp(out)))
    return float(out[0])


def locmon_compose(ref_pose4, match4, post2=(-0.275, 0.0)):
    """ndtgpu_locmon_compose: ref_pose o match o post as (x, y, c, s)"""
    a, b, c, out = _f64(ref_pose4).reshape(4), _f64(match4).reshape(4), _f64(post2).reshape(2), np.zeros(4)
    _check(lib().ndtgpu_locmon_compose(_dp(a), _dp(b), _dp(c), _dp(out)))
    return out


class LocalizationMonitor(_Handle):
    """ndtgpu_locmon: the scan-pose evaluator of flirtlib_ros over occupancy grids (include/ndtgpu.h "localisation monitor"): the
    distance field of the installed grids, the badness of (scan, grid, x, y, cos, sin) queries, adjustPose over a lattice of
    calib_lattice, and the pick of the best-matching reference scan from FeatureMatcher's device results."""
    _destroy = "ndtgpu_locmon_destroy"

    def __init__(self, max_grids, max_pixels, max_beams, max_candidates=1):
        h = C.c_void_p()
        _check(lib().ndtgpu_locmon_create(int(max_grids), int(max_pixels), int(max_beams), int(max_candidates), C.byref(h)))
        self.h = h
        self.shape = None

    def set_beams(self, n_beams, angle_min, angle_increment, stream=None):
        _check(lib().ndtgpu_locmon_set_beams(self.h, int(n_beams), float(angle_min), float(angle_increment), _stream_ptr(stream)))
        self.n_beams = int(n_beams)

    def set_grids(self, grids, resolution, origins, **params):
        """HOST grids int8 [n_grids, height, width], origins [n_grids, 2]; keyword arguments: fields of ndtgpu_locmon_params.
        Synchronous."""
        g = np.ascontiguousarray(grids, dtype=np.int8)
        if g.ndim != 3:
            raise ValueError("LocalizationMonitor.set_grids: grids must be [n_grids, height, width]")
        o = _f64(origins).reshape(-1, 2)
        if o.shape[0] != g.shape[0]:
            raise ValueError("LocalizationMonitor.set_grids: one origin per grid")
        p = locmon_params(**params)
        _check(lib().ndtgpu_locmon_set_grids(self.h, C.c_void_p(g.ctypes.data), g.shape[0], g.shape[2], g.shape[1], float(resolution), _dp(o),
                                             C.byref(p)))
        self.shape = g.shape

    def set_grids_device(self, grids_t, resolution, origins, stream=None, **params):
        """the same on a contiguous int8 device tensor [n_grids, height, width] (what MapSet.occupancy_grid_device writes),
        asynchronous on `stream`"""
        import torch
        if not (grids_t.is_cuda and grids_t.is_contiguous() and grids_t.dtype == torch.int8 and grids_t.dim() == 3):
            raise ValueError("LocalizationMonitor.set_grids_device: grids_t must be a contiguous int8 device tensor [n_grids, height, width]")
        o = _f64(origins).reshape(-1, 2)
        if o.shape[0] != grids_t.shape[0]:
            raise ValueError("LocalizationMonitor.set_grids_device: one origin per grid")
        p = locmon_params(**params)
        n, hgt, wid = (int(v) for v in grids_t.shape)
        _check(lib().ndtgpu_locmon_set_grids_device(self.h, C.c_void_p(grids_t.data_ptr()), n, wid, hgt, float(resolution), _dp(o), C.byref(p),
                                                    _stream_ptr(stream)))
        self.shape = (n, hgt, wid)

    def field(self, grid=0):
        """ndtgpu_locmon_field_get: uint16 [height, width]; 0xFFFF: no obstacle within the radius"""
        if self.shape is None:
            raise ValueError("LocalizationMonitor.field: no grids are installed")
        out = np.zeros(self.shape[1:], dtype=np.uint16)
        _check(lib().ndtgpu_locmon_field_get(self.h, int(grid), C.c_void_p(out.ctypes.data)))
        return out

    @staticmethod
    def queries(scan, grid, x, y, c, s):
        """a LOCMON_QUERY_DTYPE array from broadcastable columns"""
        cols = np.broadcast_arrays(scan, grid, x, y, c, s)
        q = np.zeros(cols[0].shape, dtype=LOCMON_QUERY_DTYPE).reshape(-1)
        for name, col in zip(("scan", "grid", "x", "y", "c", "s"), cols):
            q[name] = np.asarray(col).reshape(-1)
        return q

    def evaluate(self, ranges, queries, **params):
        """HOST ranges [n_scans, n_beams], queries LOCMON_QUERY_DTYPE [n] -> LOCMON_RESULT_DTYPE [n].  Synchronous."""
        rr = _f64(ranges)
        q = np.ascontiguousarray(queries, dtype=LOCMON_QUERY_DTYPE).reshape(-1)
        if rr.ndim != 2 or rr.shape[1] != getattr(self, "n_beams", -1):
            raise ValueError("LocalizationMonitor.evaluate: ranges must be [n_scans, n_beams of set_beams]")
        res = np.zeros(q.shape[0], dtype=LOCMON_RESULT_DTYPE)
        p = locmon_params(**params)
        _check(lib().ndtgpu_locmon_evaluate(self.h, _dp(rr), rr.shape[0], C.c_void_p(q.ctypes.data), q.shape[0], C.byref(p),
                                            C.c_void_p(res.ctypes.data)))
        return res

    def evaluate_device(self, ranges_t, queries_t, results_t, n_queries=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream`: ranges_t float64 [n_scans, n_beams] contiguous; queries_t and
        results_t contiguous device tensors of 40 and 24 bytes a record (uint8 [n, 40] / [n, 24])"""
        import torch
        if not (ranges_t.is_cuda and ranges_t.is_contiguous() and ranges_t.dtype == torch.float64 and ranges_t.dim() == 2 and
                ranges_t.shape[1] == getattr(self, "n_beams", -1)):
            raise ValueError("LocalizationMonitor.evaluate_device: ranges_t must be a contiguous float64 device tensor [n_scans, n_beams]")
        qb = queries_t.numel() * queries_t.element_size()
        n = qb // 40 if n_queries is None else int(n_queries)
        if not (queries_t.is_cuda and queries_t.is_contiguous() and qb >= 40 * n and results_t.is_cuda and results_t.is_contiguous() and
                results_t.numel() * results_t.element_size() >= 24 * n):
            raise ValueError("LocalizationMonitor.evaluate_device: queries_t / results_t must be contiguous device tensors of 40 / 24 bytes "
                             "a record")
        p = locmon_params(**params)
        _check(lib().ndtgpu_locmon_evaluate_device(self.h, C.c_void_p(ranges_t.data_ptr()), int(ranges_t.shape[0]),
                                                   C.c_void_p(queries_t.data_ptr()), n, C.byref(p), C.c_void_p(results_t.data_ptr()),
                                                   _stream_ptr(stream)))

    def adjust(self, ranges, scan, grid, lattice, want_volume=False, **params):
        """adjustPose on HOST ranges [n_scans, n_beams]: lattice is what calib_lattice(x0, y0, theta0, pos_range, pos_range, 3.14, dpos,
        dtheta) returns -> dict(index, ix, iy, iyaw, key, badness, flags, volume uint32 [nx, ny, nyaw] or None).  Synchronous."""
        rr = _f64(ranges)
        if rr.ndim != 2 or rr.shape[1] != getattr(self, "n_beams", -1):
            raise ValueError("LocalizationMonitor.adjust: ranges must be [n_scans, n_beams of set_beams]")
        xs, ys, cs, sn = _lattice_tables(lattice, "LocalizationMonitor")
        nx, ny, nyaw = xs.shape[0], ys.shape[0], cs.shape[0]
        vol = np.zeros(nx * ny * nyaw, dtype=np.uint32) if want_volume else None
        res = LocmonAdjustResult()
        p = locmon_params(**params)
        _check(lib().ndtgpu_locmon_adjust(self.h, _dp(rr), rr.shape[0], int(scan), int(grid), _dp(xs), nx, _dp(ys), ny, _dp(cs), _dp(sn), nyaw,
                                          C.byref(p), C.byref(res), None if vol is None else vol.ctypes.data_as(C.POINTER(C.c_uint32))))
        i = int(res.index)
        return dict(index=i, ix=i // (ny * nyaw), iy=(i // nyaw) % ny, iyaw=i % nyaw, key=int(res.key), badness=float(res.badness),
                    flags=int(res.flags), volume=None if vol is None else vol.reshape(nx, ny, nyaw))

    def adjust_device(self, ranges_t, scan, grid, lattice, result_t, volume_t=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream`: result_t 24 bytes (LOCMON_ADJUST_DTYPE), volume_t int32
        [nx * ny * nyaw] (read as uint32) or None"""
        import torch
        if not (ranges_t.is_cuda and ranges_t.is_contiguous() and ranges_t.dtype == torch.float64 and ranges_t.dim() == 2 and
                ranges_t.shape[1] == getattr(self, "n_beams", -1)):
            raise ValueError("LocalizationMonitor.adjust_device: ranges_t must be a contiguous float64 device tensor [n_scans, n_beams]")
        if not (result_t.is_cuda and result_t.is_contiguous() and result_t.numel() * result_t.element_size() >= 24):
            raise ValueError("LocalizationMonitor.adjust_device: result_t must be a contiguous device tensor of at least 24 bytes")
        xs, ys, cs, sn = _lattice_tables(lattice, "LocalizationMonitor")
        nc = xs.shape[0] * ys.shape[0] * cs.shape[0]
        p = locmon_params(**params)
        _check(lib().ndtgpu_locmon_adjust_device(self.h, C.c_void_p(ranges_t.data_ptr()), int(ranges_t.shape[0]), int(scan), int(grid), _dp(xs),
                                                 xs.shape[0], _dp(ys), ys.shape[0], _dp(cs), _dp(sn), cs.shape[0], C.byref(p),
                                                 C.c_void_p(result_t.data_ptr()),
                                                 _dev_ptr(volume_t, torch.int32, nc, "LocalizationMonitor.adjust_device volume_t"),
                                                 _stream_ptr(stream)))

    def pick_device(self, matches_t, ref_poses_t, n_pairs, scan, grid, query_t, pick_t, stream=None, **params):
        """ndtgpu_locmon_pick_device: matches_t the results_dev of FeatureMatcher's device match (72 bytes a record), ref_poses_t float64
        [n_pairs, 4]; writes one query (40 bytes) into query_t and one LOCMON_PICK_DTYPE record (16 bytes) into pick_t"""
        import torch
        n = int(n_pairs)
        if n and not (matches_t.is_cuda and matches_t.is_contiguous() and matches_t.numel() * matches_t.element_size() >= 72 * n):
            raise ValueError("LocalizationMonitor.pick_device: matches_t must be a contiguous device tensor of 72 bytes a pair")
        if not (query_t.is_cuda and query_t.is_contiguous() and query_t.numel() * query_t.element_size() >= 40 and pick_t.is_cuda and
                pick_t.is_contiguous() and pick_t.numel() * pick_t.element_size() >= 16):
            raise ValueError("LocalizationMonitor.pick_device: query_t / pick_t must be contiguous device tensors of 40 / 16 bytes")
        p = locmon_params(**params)
        _check(lib().ndtgpu_locmon_pick_device(self.h, C.c_void_p(matches_t.data_ptr()) if n else None,
                                               _dev_ptr(ref_poses_t, torch.float64, 4 * n, "LocalizationMonitor.pick_device ref_poses_t") if n
                                               else None, n, int(scan), int(grid), C.byref(p), C.c_void_p(query_t.data_ptr()),
                                               C.c_void_p(pick_t.data_ptr()), _stream_ptr(stream)))

    @staticmethod
    def read(t, dtype, n=1):
        """n records of `dtype` from a device tensor (synchronises through the copy to the host)"""
        import torch
        return np.frombuffer(t.view(torch.uint8).cpu().numpy().tobytes()[:dtype.itemsize * n], dtype=dtype).copy()


SCANSIM_TILE = 256           # ndtgpu_scansim_tile()
SCANSIM_OFFMAP, SCANSIM_BAD_INDEX, SCANSIM_NO_POSE = 1, 2, 4


def scansim_params(**fields):
    """ndtgpu_default_scansim_params (range_max 10, miss 11, occupied_min 55, unknown_is_obstacle 1) with fields replaced"""
    return _params(ScansimParams, "ndtgpu_default_scansim_params", "scan-simulation", fields)


def scansim_reach(range_max, resolution):
    """ndtgpu_scansim_reach: R = (int)floor(range_max / resolution), 1 .. 4094"""
    R = C.c_int32()
    _check(lib().ndtgpu_scansim_reach(float(range_max), float(resolution), C.byref(R)))
    return R.value


def scansim_skip(ref_pos_resolution, resolution):
    """ndtgpu_scansim_skip: (unsigned)(ref_pos_resolution / resolution), 1 .. 2^15"""
    k = C.c_uint32()
    _check(lib().ndtgpu_scansim_skip(float(ref_pos_resolution), float(resolution), C.byref(k)))
    return k.value


def scansim_cell(di, dj, k):
    """ndtgpu_scansim_cell -> the cell (a, b) of step k of a ray of (di, dj) cells, relative to its start"""
    cell = (C.c_int32 * 2)()
    _check(lib().ndtgpu_scansim_cell(int(di), int(dj), int(k), cell))
    return cell[0], cell[1]


def scansim_beam(grid, origin2, resolution, pose4, cb, sb, **params):
    """ndtgpu_scansim_beam: one beam on a HOST grid int8 [height, width] -> (range, hit, flags)"""
    g = np.ascontiguousarray(grid, dtype=np.int8)
    if g.ndim != 2:
        raise ValueError("scansim_beam: grid must be [height, width]")
    o, p4, r = _f64(origin2).reshape(2), _f64(pose4).reshape(4), np.zeros(1)
    hit, flags = C.c_int32(), C.c_uint32()
    p = scansim_params(**params)
    _check(lib().ndtgpu_scansim_beam(C.c_void_p(g.ctypes.data), g.shape[1], g.shape[0], _dp(o), float(resolution), _dp(p4), float(cb), float(sb),
                                     C.byref(p), _dp(r), C.byref(hit), C.byref(flags)))
    return float(r[0]), hit.value, flags.value


def scansim_headings(angle_step):
    """ndtgpu_scansim_headings -> (cs [n], sn [n]) of theta = 0, += angle_step while < 6.28"""
    n = C.c_size_t()
    _check(lib().ndtgpu_scansim_headings(float(angle_step), C.byref(n), None, None, 0))
    cs, sn = np.zeros(n.value), np.zeros(n.value)
    _check(lib().ndtgpu_scansim_headings(float(angle_step), C.byref(n), _dp(cs), _dp(sn), n.value))
    return cs, sn


class ScanSimulator(_Handle):
    """ndtgpu_scansim: occupancy_grid_utils::simulateRangeScan over installed occupancy grids and the pose lattice of flirtlib_ros'
    generateRefScans (include/ndtgpu.h "scan simulation")."""
    _destroy = "ndtgpu_scansim_destroy"

    def __init__(self, max_grids, max_beams, max_poses):
        h = C.c_void_p()
        _check(lib().ndtgpu_scansim_create(int(max_grids), int(max_beams), int(max_poses), C.byref(h)))
        self.h = h
        self.shape = None
        self._grids_t = None

    def set_beams(self, n_beams, angle_min, angle_increment, stream=None):
        _check(lib().ndtgpu_scansim_set_beams(self.h, int(n_beams), float(angle_min), float(angle_increment), _stream_ptr(stream)))
        self.n_beams = int(n_beams)

    def set_grids(self, grids, resolution, origins):
        """HOST grids int8 [n_grids, height, width], origins [n_grids, 2].  Synchronous; the handle keeps its own copy."""
        g = np.ascontiguousarray(grids, dtype=np.int8)
        if g.ndim != 3:
            raise ValueError("ScanSimulator.set_grids: grids must be [n_grids, height, width]")
        o = _f64(origins).reshape(-1, 2)
        if o.shape[0] != g.shape[0]:
            raise ValueError("ScanSimulator.set_grids: one origin per grid")
        _check(lib().ndtgpu_scansim_set_grids(self.h, C.c_void_p(g.ctypes.data), g.shape[0], g.shape[2], g.shape[1], float(resolution), _dp(o)))
        self.shape = g.shape
        self._grids_t = None

    def set_grids_device(self, grids_t, resolution, origins, stream=None):
        """the same on a contiguous int8 device tensor [n_grids, height, width] (what MapSet.occupancy_grid_device writes),
        asynchronous on `stream`.  The bytes are BORROWED: this object keeps the tensor alive until the next set or close."""
        import torch
        if not (grids_t.is_cuda and grids_t.is_contiguous() and grids_t.dtype == torch.int8 and grids_t.dim() == 3):
            raise ValueError("ScanSimulator.set_grids_device: grids_t must be a contiguous int8 device tensor [n_grids, height, width]")
        o = _f64(origins).reshape(-1, 2)
        if o.shape[0] != grids_t.shape[0]:
            raise ValueError("ScanSimulator.set_grids_device: one origin per grid")
        n, hgt, wid = (int(v) for v in grids_t.shape)
        _check(lib().ndtgpu_scansim_set_grids_device(self.h, C.c_void_p(grids_t.data_ptr()), n, wid, hgt, float(resolution), _dp(o),
                                                     _stream_ptr(stream)))
        self.shape = (n, hgt, wid)
        self._grids_t = grids_t

    def close(self):
        super().close()
        self._grids_t = None

    @staticmethod
    def _headings(headings):
        cs, sn = (_f64(a).reshape(-1) for a in headings)
        if cs.shape != sn.shape:
            raise ValueError("ScanSimulator: headings must be (cs [nyaw], sn [nyaw])")
        return cs, sn

    @staticmethod
    def _box(box):
        return None if box is None else _f64(box).reshape(4)

    def lattice(self, skip, headings, capacity, grid=0, box=None, want_index=True):
        """generateRefScans' lattice into HOST arrays: headings = (cs, sn) of scansim_headings, box = (x0, y0, x1, y1) or None ->
        dict(poses [written, 4], index uint32 [written] or None, written, passed).  Synchronous."""
        cs, sn = self._headings(headings)
        b = self._box(box)
        poses = np.zeros((int(capacity), 4))
        index = np.zeros(int(capacity), dtype=np.uint32) if want_index else None
        counts = (C.c_uint32 * 2)()
        _check(lib().ndtgpu_scansim_lattice(self.h, int(grid), int(skip), _dp(cs), _dp(sn), cs.shape[0], None if b is None else _dp(b),
                                            int(capacity), _dp(poses), None if index is None else index.ctypes.data_as(C.POINTER(C.c_uint32)),
                                            counts))
        n = int(counts[0])
        return dict(poses=poses[:n], index=None if index is None else index[:n], written=n, passed=int(counts[1]))

    def lattice_device(self, skip, headings, capacity, poses_t, count_t, index_t=None, grid=0, box=None, stream=None):
        """the same on torch device tensors, asynchronous on `stream`: poses_t float64 [capacity, 4], count_t int32 [2] (read as
        uint32: written, passed), index_t int32 [capacity] or None"""
        import torch
        cs, sn = self._headings(headings)
        b = self._box(box)
        _check(lib().ndtgpu_scansim_lattice_device(self.h, int(grid), int(skip), _dp(cs), _dp(sn), cs.shape[0], None if b is None else _dp(b),
                                                   int(capacity),
                                                   _dev_ptr(poses_t, torch.float64, 4 * int(capacity), "ScanSimulator.lattice_device poses_t"),
                                                   _dev_ptr(index_t, torch.int32, int(capacity), "ScanSimulator.lattice_device index_t"),
                                                   _dev_ptr(count_t, torch.int32, 2, "ScanSimulator.lattice_device count_t"),
                                                   _stream_ptr(stream)))

    def simulate(self, poses, grid_idx=None, want_results=True, **params):
        """HOST poses [n, 4] = (x, y, cos, sin), grid_idx [n] or None: grid 0 -> (ranges [n, n_beams], SCANSIM_RESULT_DTYPE [n] or
        None); keyword arguments: fields of ndtgpu_scansim_params.  Synchronous."""
        pp = _f64(poses).reshape(-1, 4)
        n = pp.shape[0]
        gi = None if grid_idx is None else np.ascontiguousarray(grid_idx, dtype=np.uint32).reshape(-1)
        if gi is not None and gi.shape[0] != n:
            raise ValueError("ScanSimulator.simulate: one grid index per pose")
        ranges = np.zeros((n, getattr(self, "n_beams", 0)))
        res = np.zeros(n, dtype=SCANSIM_RESULT_DTYPE) if want_results else None
        p = scansim_params(**params)
        _check(lib().ndtgpu_scansim_simulate(self.h, _dp(pp), None if gi is None else gi.ctypes.data_as(C.POINTER(C.c_uint32)), n, C.byref(p),
                                             _dp(ranges), None if res is None else C.c_void_p(res.ctypes.data)))
        return ranges, res

    def simulate_device(self, poses_t, ranges_t, n_poses=None, grid_idx_t=None, count_t=None, results_t=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream`: poses_t float64 [n, 4]; ranges_t float64 [n, n_beams]; grid_idx_t
        int32 [n] or None; count_t int32 [>= 1] or None (rows at or beyond count_t[0] become NO_POSE scans); results_t a contiguous
        device tensor of 8 bytes a pose or None"""
        import torch
        n = int(poses_t.shape[0]) if n_poses is None else int(n_poses)
        nb = getattr(self, "n_beams", 0)
        if results_t is not None and not (results_t.is_cuda and results_t.is_contiguous() and results_t.numel() * results_t.element_size() >= 8 * n):
            raise ValueError("ScanSimulator.simulate_device: results_t must be a contiguous device tensor of 8 bytes a pose")
        p = scansim_params(**params)
        _check(lib().ndtgpu_scansim_simulate_device(self.h, _dev_ptr(poses_t, torch.float64, 4 * n, "ScanSimulator.simulate_device poses_t"),
                                                    _dev_ptr(grid_idx_t, torch.int32, n, "ScanSimulator.simulate_device grid_idx_t"), n,
                                                    _dev_ptr(count_t, torch.int32, 1, "ScanSimulator.simulate_device count_t"), C.byref(p),
                                                    _dev_ptr(ranges_t, torch.float64, n * nb, "ScanSimulator.simulate_device ranges_t"),
                                                    None if results_t is None else C.c_void_p(results_t.data_ptr()), _stream_ptr(stream)))

    @staticmethod
    def read(t, dtype, n=1):
        """n records of `dtype` from a device tensor (synchronises through the copy to the host)"""
        import torch
        return np.frombuffer(t.view(torch.uint8).cpu().numpy().tobytes()[:dtype.itemsize * n], dtype=dtype).copy()


def match_d2d(target_set, tmap, source_set, smap, T, **params):
    To, res = match_batch(target_set, [tmap], source_set, [smap], np.asarray(T)[None], **params)
    return To[0], res[0]


def overlap_score(ref_set, ref_idx, mov_set, mov_idx, T, stream=None):
    """ndt_feature::overlapNDTOccupancyScore(ref, mov, T) for every link -> (scores [n], nb_sum [n])."""
    ri = np.ascontiguousarray(ref_idx, dtype=np.uint32)
    mi = np.ascontiguousarray(mov_idx, dtype=np.uint32)
    n = ri.shape[0]
    Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
    score = np.zeros(n)
    nb = np.zeros(n, dtype=np.int64)
    _check(lib().ndtgpu_overlap_score_batch(ref_set.h, ri.ctypes.data_as(C.POINTER(C.c_uint32)), mov_set.h,
                                            mi.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(Tc), n, _dp(score),
                                            nb.ctypes.data_as(C.POINTER(C.c_int64)), _stream_ptr(stream)))
    return score, nb


def covariance(target_set, target_idx, source_set, source_idx, T, mode=0, stream=None, **params):
    """NDTMatcherD2D::covariance(target, source, T, cov) for every link -> (cov [n,6,6], singular [n])."""
    ti = np.ascontiguousarray(target_idx, dtype=np.uint32)
    si = np.ascontiguousarray(source_idx, dtype=np.uint32)
    n = ti.shape[0]
    Tc = np.ascontiguousarray(np.transpose(np.asarray(T, dtype=np.float64).reshape(n, 4, 4), (0, 2, 1))).copy()
    cov = np.zeros((n, 6, 6))
    sing = np.zeros(n, dtype=np.int32)
    p = match_params(**params)
    _check(lib().ndtgpu_covariance_batch(target_set.h, ti.ctypes.data_as(C.POINTER(C.c_uint32)), source_set.h,
                                         si.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(Tc), n, C.byref(p), int(mode), _dp(cov),
                                         sing.ctypes.data_as(C.POINTER(C.c_int32)), _stream_ptr(stream)))
    return cov, sing


MARKER_TILE = 256            # ndtgpu_marker_tile()
MARKER_NONFINITE, MARKER_BAD_INDEX = 1, 2
MARKER_SCALE_X = 0.02        # scale.x of the LINE_LIST markers (ndt_rviz.h)


def marker_params(**fields):
    """ndtgpu_default_marker_params (min_eval 0.0001, particle_length 0.3, skip_negative 0) with fields replaced"""
    return _params(MarkerParams, "ndtgpu_default_marker_params", "marker", fields, hidden=("reserved",))


def _cm16(T):
    """[n, 4, 4] math convention -> [n, 16] column-major"""
    T = _f64(T).reshape(-1, 4, 4)
    return np.ascontiguousarray(np.transpose(T, (0, 2, 1))).reshape(-1, 16)


def marker_eig3(cov):
    """ndtgpu_marker_eig3 (host): cov [3, 3] symmetric or [6] = (xx xy xz yy yz zz) -> (evals [3] ascending, V [3, 3], column j the
    unit eigenvector of evals[j], its largest component positive)"""
    c = _f64(cov).reshape(-1)
    if c.shape[0] == 9:
        c = c[[0, 1, 2, 4, 5, 8]].copy()
    if c.shape[0] != 6:
        raise ValueError("marker_eig3: cov must be [3, 3] or [6]")
    ev, V = np.zeros(3), np.zeros(9)
    _check(lib().ndtgpu_marker_eig3(_dp(c), _dp(ev), _dp(V)))
    return ev, V.reshape(3, 3)


def marker_cell(mean, cov, pose=None, **params):
    """ndtgpu_marker_cell (host): the segments of one cell -> (seg [n_seg, 2, 3], evals [3], flags); pose: [4, 4] or None"""
    m, c = _f64(mean).reshape(3), _f64(cov).reshape(-1)
    if c.shape[0] == 9:
        c = c[[0, 1, 2, 4, 5, 8]].copy()
    if c.shape[0] != 6:
        raise ValueError("marker_cell: cov must be [3, 3] or [6]")
    T = None if pose is None else _cm16(pose)
    seg, ev = np.zeros(18), np.zeros(3)
    n, flags = C.c_uint32(), C.c_uint32()
    p = marker_params(**params)
    _check(lib().ndtgpu_marker_cell(_dp(m), _dp(c), None if T is None else _dp(T), C.byref(p), _dp(seg), _dp(ev), C.byref(n), C.byref(flags)))
    return seg.reshape(3, 2, 3)[:n.value].copy(), ev, flags.value


class Marker(_Handle):
    """ndtgpu_marker: the tile words and count words of a marker selection (include/ndtgpu.h "marker export")."""
    _destroy = "ndtgpu_marker_destroy"

    def __init__(self, max_maps_per_call, max_links=0):
        h = C.c_void_p()
        _check(lib().ndtgpu_marker_create(int(max_maps_per_call), int(max_links), C.byref(h)))
        self.h = h

    def count(self):
        """(n_segments, overflow, flags) of the last cell or link call; waits for the handle"""
        n, o, f = C.c_size_t(), C.c_int32(), C.c_uint32()
        _check(lib().ndtgpu_marker_count(self.h, C.byref(n), C.byref(o), C.byref(f)))
        return int(n.value), bool(o.value), int(f.value)

    def cells(self, map_set, first, count, poses=None, capacity=0, want_src=True, **params):
        """MapSet.markers with this handle"""
        first, count, cap = int(first), int(count), int(capacity)
        T = None
        if poses is not None:
            T = _cm16(poses)
            if T.shape[0] != count:
                raise ValueError("markers: one pose per map")
        pts = np.zeros((max(cap, 1), 6))
        src = np.zeros((max(cap, 1), 2), dtype=np.uint32) if want_src else None
        n, o, f = C.c_size_t(), C.c_int32(), C.c_uint32()
        p = marker_params(**params)
        _check(lib().ndtgpu_mapset_markers(self.h, map_set.h, first, count, None if T is None or count == 0 else _dp(T), C.byref(p),
                                           _dp(pts) if cap else None,
                                           src.ctypes.data_as(C.POINTER(C.c_uint32)) if want_src and cap else None, cap, C.byref(n),
                                           C.byref(o), C.byref(f)))
        m = min(int(n.value), cap)
        return (pts[:m].reshape(m, 2, 3), None if src is None else src[:m],
                dict(n_segments=int(n.value), overflow=bool(o.value), flags=int(f.value)))

    def cells_device(self, map_set, first, count, points_t, src_t=None, poses_t=None, capacity=None, stream=None, **params):
        """MapSet.markers_device with this handle"""
        import torch
        count = int(count)
        cap = points_t.numel() // 6 if capacity is None else int(capacity)
        p = marker_params(**params)
        _check(lib().ndtgpu_mapset_markers_device(self.h, map_set.h, int(first), count,
                                                  _dev_ptr(poses_t, torch.float64, 16 * count, "markers_device poses_t"), C.byref(p),
                                                  _dev_ptr(points_t, torch.float64, 6 * cap, "markers_device points_t"),
                                                  _dev_ptr(src_t, torch.int32, 2 * cap, "markers_device src_t"), cap, _stream_ptr(stream)))

    def links(self, poses, ref, mov, score=None, capacity=None, **params):
        """markerNDTFeatureLinks on HOST arrays: poses [n_nodes, 4, 4], ref / mov [n_links], score [n_links] or None -> (points [n, 2,
        3], info dict(n_segments, overflow)); skip_negative=1 skips links with score < 0.  Synchronous."""
        T = _cm16(poses)
        r = np.ascontiguousarray(ref, dtype=np.uint32).reshape(-1)
        m = np.ascontiguousarray(mov, dtype=np.uint32).reshape(-1)
        if r.shape != m.shape:
            raise ValueError("link_markers: one ref and one mov index per link")
        sc = None if score is None else _f64(score).reshape(-1)
        if sc is not None and sc.shape != r.shape:
            raise ValueError("link_markers: one score per link")
        cap = r.shape[0] if capacity is None else int(capacity)
        pts = np.zeros((max(cap, 1), 6))
        n, o = C.c_size_t(), C.c_int32()
        p = marker_params(**params)
        u32p = C.POINTER(C.c_uint32)
        _check(lib().ndtgpu_marker_links(self.h, _dp(T) if T.shape[0] else None, T.shape[0], r.ctypes.data_as(u32p), m.ctypes.data_as(u32p),
                                         None if sc is None else _dp(sc), r.shape[0], C.byref(p), _dp(pts) if cap else None, cap, C.byref(n),
                                         C.byref(o)))
        k = min(int(n.value), cap)
        return pts[:k].reshape(k, 2, 3), dict(n_segments=int(n.value), overflow=bool(o.value))

    def links_device(self, poses_t, ref_t, mov_t, points_t, score_t=None, n_links=None, capacity=None, stream=None, **params):
        """the same on torch device tensors, asynchronous on `stream`: poses_t float64 [n_nodes, 16] column-major, ref_t / mov_t int32
        (read as uint32), score_t float64 or None, points_t float64 [capacity, 6]; the counts stay with the handle (count())"""
        import torch
        n_nodes = poses_t.numel() // 16
        m = ref_t.numel() if n_links is None else int(n_links)
        cap = points_t.numel() // 6 if capacity is None else int(capacity)
        p = marker_params(**params)
        _check(lib().ndtgpu_marker_links_device(self.h, _dev_ptr(poses_t, torch.float64, 16 * n_nodes, "links_device poses_t"), n_nodes,
                                                _dev_ptr(ref_t, torch.int32, m, "links_device ref_t"),
                                                _dev_ptr(mov_t, torch.int32, m, "links_device mov_t"),
                                                _dev_ptr(score_t, torch.float64, m, "links_device score_t"), m, C.byref(p),
                                                _dev_ptr(points_t, torch.float64, 6 * cap, "links_device points_t"), cap, _stream_ptr(stream)))


def link_markers(poses, ref, mov, score=None, capacity=None, **params):
    """Marker.links with a handle made for the call"""
    n = int(np.asarray(ref).size)
    mk = Marker(1, max(n, 1))
    try:
        return mk.links(poses, ref, mov, score=score, capacity=capacity, **params)
    finally:
        mk.close()
