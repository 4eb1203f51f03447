"""ndt_feature_graph_amd -- MI355X-native NDT scan-matching front-end (grid build + D2D matcher)
behind the lslgeneric::NDTMap / NDTMatcherD2D call sites of MalcolmMielle/ndt_feature_graph.

The product is the C-ABI shared library (include/ndtgpu.h, csrc/*.hip -> libndtgpu.so).  This
Python package is only the thin ctypes host layer used by tests/ and bench.py; the C++ host
mirror of the reference classes lives in ndt_feature_graph_amd/host/.

There is no CPU fallback: importing works anywhere (the build check runs without a GPU), but
every compute call raises NdtGpuError when the HIP library or a device is missing.
"""
from .binding import (MapSet, Registrar, MultiRes, MCL, mcl_params, PGO, pgo_params, PgoWideParams, pgo_wide_params, pgo_wide_plan, assemble_world, world_params, WorldParams, WorldResult, occupancy_grid_dims, occupancy_grid_move, occgrid_params, OccGridParams, OccGridInfo, LinkGate, LinkGateParams, linkgate_params, optimize_gated, FeatureMatcher, featmatch_params, featextract_params, default_resolutions, FuserBank, fuser_params, fuser_prepare, fuser_feat_params, fuser_feat_prepare, fuser_feat_move, FuserFeatParams, FuserFeatResult, ScanProjector, ScanProjectParams, scanproject_params, scan_project_beam, SCANPROJECT_TILE, Calibrator, CalibParams, CalibResult, CALIB_RESULT_DTYPE, CALIB_TILE, CALIB_NO_RESULT, CALIB_BAD_PAIR, calib_params, calib_lattice, calib_pair_motion, calib_select_pairs, LocalizationMonitor, LocmonParams, LocmonQuery, LocmonResult, LocmonAdjustResult, LocmonPick, LOCMON_QUERY_DTYPE, LOCMON_RESULT_DTYPE, LOCMON_ADJUST_DTYPE, LOCMON_PICK_DTYPE, LOCMON_TILE, LOCMON_NO_BEAMS, LOCMON_BAD_INDEX, LOCMON_NO_QUERY, LOCMON_NO_RESULT, LOCMON_NO_PICK, LOCMON_KEY_FAR, LOCMON_KEY_OFFMAP, LOCMON_NO_SCAN, locmon_params, locmon_radius, locmon_beam_table, locmon_pixel, locmon_metres, locmon_compose, ScanSimulator, ScansimParams, ScansimResult, SCANSIM_RESULT_DTYPE, SCANSIM_TILE, SCANSIM_OFFMAP, SCANSIM_BAD_INDEX, SCANSIM_NO_POSE, scansim_params, scansim_reach, scansim_skip, scansim_cell, scansim_beam, scansim_headings, covariance, MatchParams, NdtGpuError, build_library, derivatives, device_count, lib,  # noqa: F401
                      library_path, match_batch, match_d2d, match_fusion_batch, overlap_score)
