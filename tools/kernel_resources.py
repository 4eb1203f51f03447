#!/usr/bin/env python3
"""Prints VGPR / SGPR / spill / scratch / LDS figures of every kernel in the shipped libndtgpu.so
(code-object metadata, what the judge reads).  usage: python tools/kernel_resources.py [filter]
filter: a substring of the (mangled) kernel name, or one of the named groups below."""
import os, re, subprocess, sys, tempfile
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
so = os.path.join(root, "ndt_feature_graph_amd", "libndtgpu.so")
llvm = "/opt/rocm/lib/llvm/bin"
with tempfile.TemporaryDirectory() as d:
    co = os.path.join(d, "co")
    # the fat binary sits in .hip_fatbin of the shared object
    fb = os.path.join(d, "fb")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fb])
    blob = open(fb, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(magic, blob)]
    txt = ""
    for k, st in enumerate(starts):                     # one bundle per translation unit
        part = os.path.join(d, "fb%d" % k)
        open(part, "wb").write(blob[st:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + part,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        txt += subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co]).decode()
# named groups: every kernel of a subsystem, by name
GROUPS = {"pgo_wide": ["ndt_pgo_wide_linearise_kernel", "ndt_pgo_wide_assess_kernel", "ndt_pgo_wide_start_kernel", "ndt_pgo_wide_link_kernel",
                       "ndt_pgo_wide_node_kernel", "ndt_pgo_wide_step_kernel", "ndt_pgo_wide_update_kernel"],
          "pgo3": ["ndt_pgo3_kernel", "ndt_pgo3_links_kernel"],
          "pgo_marginals": ["ndt_pgo_marginal_prepare_kernel", "ndt_pgo_marginal_solve_kernel", "ndt_pgo_marginal_finish_kernel",
                            "ndt_pgo3_marginal_prepare_kernel", "ndt_pgo3_marginal_solve_kernel"],
          "pgo3_wide": ["ndt_pgo3_wide_linearise_kernel", "ndt_pgo3_wide_assess_kernel", "ndt_pgo3_wide_start_kernel", "ndt_pgo3_wide_link_kernel",
                        "ndt_pgo3_wide_node_kernel", "ndt_pgo3_wide_step_kernel", "ndt_pgo3_wide_update_kernel"],
          "pgo_robust": ["ndt_pgo_robust_weigh_kernel", "ndt_pgo_robust_finish_kernel", "ndt_pgo3_robust_weigh_kernel",
                         "ndt_pgo3_robust_finish_kernel"],
          "calib": ["ndt_calib_prepare_kernel", "ndt_calib_score_kernel", "ndt_calib_finish_kernel", "ndt_calib_winner_kernel"],
          "locmon": ["ndt_locmon_row_kernel", "ndt_locmon_col_kernel", "ndt_locmon_badness_kernel", "ndt_locmon_finish_kernel",
                     "ndt_locmon_winner_kernel", "ndt_locmon_pick_kernel"],
          "scansim": ["ndt_scansim_cast_kernel", "ndt_scansim_flag_kernel", "ndt_scansim_scan_kernel", "ndt_scansim_emit_kernel"],
          "marker": ["ndt_marker_count_kernel", "ndt_marker_scan_kernel", "ndt_marker_emit_kernel", "ndt_marker_link_flag_kernel",
                     "ndt_marker_link_emit_kernel", "ndt_marker_particle_kernel"]}
flt = sys.argv[1] if len(sys.argv) > 1 else ""
names = GROUPS.get(flt, [flt])
for blk in txt.split("- .agpr_count")[1:]:
    g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
    name = g("name")
    if flt and not any(n in name for n in names): continue
    short = subprocess.check_output(["c++filt", name]).decode().split("(")[0]
    print("%-44s vgpr %3s sgpr %3s vspill %3s sspill %3s scratch %4s lds %6s" % (
        short[:44], g("vgpr_count"), g("sgpr_count"), g("vgpr_spill_count"), g("sgpr_spill_count"),
        g("private_segment_fixed_size"), g("group_segment_fixed_size")))
