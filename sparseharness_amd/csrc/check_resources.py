#!/usr/bin/env python3
"""Reads hipcc's -Rpass-analysis=kernel-resource-usage remarks and fails if a kernel of the tiled plan, or one of the
multi-vector kernels (spmm_csr_kernel / spmm_long_fixup, multi.hip.h), or one of the packed-bit kernels (msbfs_csr_kernel /
msbfs_long_fixup, msbfs.hip.h), or one of the frontier kernels (frontier_mark / frontier_pull / frontier_apply /
frontier_detect, frontier.hip.h), or one of the BFS kernels (bfs_init / bfs_topdown / bfs_bottomup / bfs_queue_from_bitmap /
bfs_decide / bfs_parents, bfs.hip.h), or one of the SSSP kernels (sssp_init / sssp_relax / sssp_split / sssp_decide /
sssp_preds, sssp.hip.h), or one of the SCC kernels (scc_init / scc_trim / scc_pick / scc_seed / scc_propagate / scc_claim /
scc_label / scc_decide, scc.hip.h), or one of the WCC kernels (wcc_init / wcc_sample / wcc_compact / wcc_full / wcc_jump /
wcc_decide / wcc_label, wcc.hip.h), or one of the triangle kernels (tri_count_light / tri_count_heavy, each with and without
per-vertex counts, and tri_finish, tri.hip.h), or one of the core-number kernels (core_init / core_min / core_open / core_peel /
core_close, core.hip.h), or one of the truss kernels (truss_init / truss_support / truss_total / truss_min / truss_open /
truss_peel / truss_close, truss.hip.h), or one of the colouring kernels (gcol_init / gcol_count / gcol_ready / gcol_assign /
gcol_close, color.hip.h; the prefix is their own because scc.hip.h speaks of colouring too), or one of the spanning-forest
kernels (msf_weights / msf_init / msf_find / msf_pick / msf_link / msf_jump / msf_close / msf_top / msf_label, msf.hip.h), or one of the matching
kernels (match_init / match_bid / match_take / match_clear / match_close, match.hip.h), or one of the ordering kernels (rcm_init /
rcm_begin / rcm_sweep / rcm_claim / rcm_count / rcm_place / rcm_close / rcm_finish / rcm_total, rcm.hip.h), or one of the betweenness
kernels (bc_in_keys / bc_out_keys / bc_init / bc_expand / bc_count / bc_close / bc_delta, bc.hip.h), or one of the triangular-solve
kernels (trsv_flag / trsv_keys / trsv_diag / trsv_flip / trsv_seed / trsv_settle / trsv_close / trsv_rank_keys / trsv_order /
trsv_level / trsv_run, trsv.hip.h), or one of the incomplete-LU kernels (ilu0_flag / ilu0_keys / ilu0_slots / ilu0_diag /
ilu0_work / ilu0_load / ilu0_level / ilu0_run / ilu0_store, ilu0.hip.h), uses scratch or spills VGPRs or SGPRs (see the asm-check target of the Makefile)."""
import re
import sys

text = open(sys.argv[1]).read()
bad, seen, seen_multi, seen_bits, seen_frontier, seen_bfs, seen_sssp, seen_scc, seen_wcc, seen_tri, seen_core, seen_truss, seen_gcol, seen_msf, seen_match, seen_rcm, seen_bc, seen_trsv, seen_ilu0 = [], 0, set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set(), set()
BFS_KERNELS = ("bfs_init", "bfs_topdown", "bfs_bottomup", "bfs_queue_from_bitmap", "bfs_decide", "bfs_parents")
SSSP_KERNELS = ("sssp_init", "sssp_relax", "sssp_split", "sssp_decide", "sssp_preds")
SCC_KERNELS = ("scc_init", "scc_trim", "scc_pick", "scc_seed", "scc_propagate", "scc_claim", "scc_label", "scc_decide")
TRI_KERNELS = ("tri_count_light", "tri_count_heavy", "tri_finish")
CORE_KERNELS = ("core_init", "core_min", "core_open", "core_peel", "core_close")
TRUSS_KERNELS = ("truss_init", "truss_support", "truss_total", "truss_min", "truss_open", "truss_peel", "truss_close")
GCOL_KERNELS = ("gcol_init", "gcol_count", "gcol_ready", "gcol_assign", "gcol_close")
MATCH_KERNELS = ("match_init", "match_bid", "match_take", "match_clear", "match_close")
RCM_KERNELS = ("rcm_init", "rcm_begin", "rcm_sweep", "rcm_claim", "rcm_count", "rcm_place", "rcm_close", "rcm_finish", "rcm_total")
BC_KERNELS = ("bc_in_keys", "bc_out_keys", "bc_init", "bc_expand", "bc_count", "bc_close", "bc_delta")
TRSV_KERNELS = ("trsv_flag", "trsv_keys", "trsv_diag", "trsv_flip", "trsv_seed", "trsv_settle", "trsv_close", "trsv_rank_keys",
                "trsv_order", "trsv_level", "trsv_run")
ILU0_KERNELS = ("ilu0_flag", "ilu0_keys", "ilu0_slots", "ilu0_diag", "ilu0_work", "ilu0_load", "ilu0_level", "ilu0_run", "ilu0_store")
MSF_KERNELS = ("msf_weights", "msf_init", "msf_find", "msf_pick", "msf_link", "msf_jump", "msf_close", "msf_top", "msf_label")
WCC_KERNELS = ("wcc_init", "wcc_sample", "wcc_compact", "wcc_full", "wcc_jump", "wcc_decide", "wcc_label")
for blk in text.split("remark: Function Name: ")[1:]:
    name = blk.split()[0]
    multi = "spmm_csr" in name or "spmm_long" in name
    packed = "msbfs_csr" in name or "msbfs_long" in name
    frontier = any(k in name for k in ("frontier_mark", "frontier_pull", "frontier_apply", "frontier_detect"))
    bfs = any(k in name for k in BFS_KERNELS)
    sssp = any(k in name for k in SSSP_KERNELS)
    scc = any(k in name for k in SCC_KERNELS)
    wcc = any(k in name for k in WCC_KERNELS)
    tri = any(k in name for k in TRI_KERNELS)
    core = any(k in name for k in CORE_KERNELS)
    truss = any(k in name for k in TRUSS_KERNELS)
    gcol = any(k in name for k in GCOL_KERNELS)
    msf = any(k in name for k in MSF_KERNELS)
    match = any(k in name for k in MATCH_KERNELS)
    rcm = any(k in name for k in RCM_KERNELS)
    bc = any(k in name for k in BC_KERNELS)
    trsv = any(k in name for k in TRSV_KERNELS)
    ilu0 = any(k in name for k in ILU0_KERNELS)
    if "spmv_tiled" not in name and not multi and not packed and not frontier and not bfs and not sssp and not scc and not wcc and not tri and not core and not truss and not gcol and not msf and not match and not rcm and not bc and not trsv and not ilu0:
        continue
    if ilu0:
        seen_ilu0.add(name)
    elif trsv:
        seen_trsv.add(name)
    elif bc:
        seen_bc.add(name)
    elif rcm:
        seen_rcm.add(name)
    elif match:
        seen_match.add(name)
    elif msf:
        seen_msf.add(name)
    elif gcol:
        seen_gcol.add(name)
    elif truss:
        seen_truss.add(name)
    elif core:
        seen_core.add(name)
    elif tri:
        seen_tri.add(name)
    elif wcc:
        seen_wcc.add(name)
    elif scc:
        seen_scc.add(name)
    elif sssp:
        seen_sssp.add(name)
    elif bfs:
        seen_bfs.add(name)
    elif frontier:
        seen_frontier.add(name)
    elif multi:
        seen_multi.add(name)
    elif packed:
        seen_bits.add(name)
    else:
        seen += 1
    scratch = int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk).group(1))
    spill = int(re.search(r"VGPRs Spill: (\d+)", blk).group(1))
    vgprs = int(re.search(r"VGPRs: (\d+)", blk).group(1))
    sspill = int(re.search(r"SGPRs Spill: (\d+)", blk).group(1))
    # 1024-thread workgroups: 128 VGPRs per lane is all there is.  The experimental fused kernel may carry a
    # scavenger slot (a few bytes of private segment that no instruction touches: checked in the .s once); the
    # default kernels must have none.
    # (a spilled SGPR lives in a lane of a VGPR the hand-scheduled loaders might otherwise count on, and costs
    # v_writelane / v_readlane traffic wherever it is used)
    # The multi-vector kernels run 256-thread workgroups, four per CU by their LDS (40 KB each): 16 waves per CU, four
    # per SIMD, which 128 VGPRs per lane still allow -- the same bound.  The packed-bit kernels stage half as much (22 KB):
    # seven workgroups per CU, 28 waves, seven per SIMD: 512 / 7 = 73 VGPRs would be the limit for that; they are held to 64.
    if spill or sspill or vgprs > (64 if packed else 128) or scratch:
        bad.append((name, scratch, spill, vgprs, sspill))
if not seen:
    sys.exit("no spmv_tiled kernels found in the resource-usage remarks")
# four semirings x four widths of spmm_csr_kernel, and as many fix-up kernels
n_csr = sum("spmm_csr" in n for n in seen_multi)
if n_csr != 16 or len(seen_multi) != 32:
    sys.exit(f"expected 16 spmm_csr_kernel and 16 spmm_long_fixup instantiations in the remarks, found {n_csr} and {len(seen_multi) - n_csr}")
# four `words` x {plain, with level counts} of msbfs_csr_kernel, and as many fix-up kernels
n_bits = sum("msbfs_csr" in n for n in seen_bits)
if n_bits != 8 or len(seen_bits) != 16:
    sys.exit(f"expected 8 msbfs_csr_kernel and 8 msbfs_long_fixup instantiations in the remarks, found {n_bits} and {len(seen_bits) - n_bits}")
# frontier_mark, frontier_detect, and frontier_pull / frontier_apply for the three order-free semirings
if len(seen_frontier) != 8:
    sys.exit(f"expected 8 frontier kernels in the remarks, found {len(seen_frontier)}: {sorted(seen_frontier)}")
# the six kernels of sh_bfs_levels, under the limits of the frontier kernels
if len(seen_bfs) != len(BFS_KERNELS):
    sys.exit(f"expected {len(BFS_KERNELS)} BFS kernels in the remarks, found {len(seen_bfs)}: {sorted(seen_bfs)}")
# the five kernels of sh_sssp, under the limits of the BFS kernels
if len(seen_sssp) != len(SSSP_KERNELS):
    sys.exit(f"expected {len(SSSP_KERNELS)} SSSP kernels in the remarks, found {len(seen_sssp)}: {sorted(seen_sssp)}")
# the eight kernels of sh_scc, under the limits of the BFS kernels
if len(seen_scc) != len(SCC_KERNELS):
    sys.exit(f"expected {len(SCC_KERNELS)} SCC kernels in the remarks, found {len(seen_scc)}: {sorted(seen_scc)}")
# the seven kernels of sh_wcc, under the limits of the BFS kernels
if len(seen_wcc) != len(WCC_KERNELS):
    sys.exit(f"expected {len(WCC_KERNELS)} WCC kernels in the remarks, found {len(seen_wcc)}: {sorted(seen_wcc)}")
# the two counting kernels of sh_tri with and without per-vertex counts and tri_finish, under the limits of the BFS kernels
if len(seen_tri) != 5:
    sys.exit(f"expected 5 triangle kernels in the remarks, found {len(seen_tri)}: {sorted(seen_tri)}")
# the five kernels of sh_core, under the limits of the BFS kernels
if len(seen_core) != len(CORE_KERNELS):
    sys.exit(f"expected {len(CORE_KERNELS)} core-number kernels in the remarks, found {len(seen_core)}: {sorted(seen_core)}")
# the seven kernels of sh_truss, under the limits of the BFS kernels
if len(seen_truss) != len(TRUSS_KERNELS):
    sys.exit(f"expected {len(TRUSS_KERNELS)} truss kernels in the remarks, found {len(seen_truss)}: {sorted(seen_truss)}")
# the five kernels of sh_color, under the limits of the BFS kernels
if len(seen_gcol) != len(GCOL_KERNELS):
    sys.exit(f"expected {len(GCOL_KERNELS)} colouring kernels in the remarks, found {len(seen_gcol)}: {sorted(seen_gcol)}")
# the nine kernels of sh_msf, under the limits of the BFS kernels
if len(seen_msf) != len(MSF_KERNELS):
    sys.exit(f"expected {len(MSF_KERNELS)} spanning-forest kernels in the remarks, found {len(seen_msf)}: {sorted(seen_msf)}")
# the five kernels of sh_match, under the limits of the BFS kernels
if len(seen_match) != len(MATCH_KERNELS):
    sys.exit(f"expected {len(MATCH_KERNELS)} matching kernels in the remarks, found {len(seen_match)}: {sorted(seen_match)}")
# the nine kernels of sh_rcm, under the limits of the BFS kernels
if len(seen_rcm) != len(RCM_KERNELS):
    sys.exit(f"expected {len(RCM_KERNELS)} ordering kernels in the remarks, found {len(seen_rcm)}: {sorted(seen_rcm)}")
# the seven kernels of sh_bc, under the limits of the BFS kernels
if len(seen_bc) != len(BC_KERNELS):
    sys.exit(f"expected {len(BC_KERNELS)} betweenness kernels in the remarks, found {len(seen_bc)}: {sorted(seen_bc)}")
# the eleven kernels of sh_trsv, under the limits of the BFS kernels
if len(seen_trsv) != len(TRSV_KERNELS):
    sys.exit(f"expected {len(TRSV_KERNELS)} triangular-solve kernels in the remarks, found {len(seen_trsv)}: {sorted(seen_trsv)}")
# the nine kernels of sh_ilu0, under the limits of the BFS kernels
if len(seen_ilu0) != len(ILU0_KERNELS):
    sys.exit(f"expected {len(ILU0_KERNELS)} incomplete-LU kernels in the remarks, found {len(seen_ilu0)}: {sorted(seen_ilu0)}")
for b in bad:
    print("resource check FAILED: %s scratch=%d vgpr_spill=%d vgprs=%d sgpr_spill=%d" % b)
print(f"{seen} tiled, {len(seen_multi)} multi-vector, {len(seen_bits)} packed-bit, {len(seen_frontier)} frontier, {len(seen_bfs)} BFS, {len(seen_sssp)} SSSP, {len(seen_scc)} SCC, {len(seen_wcc)} WCC, {len(seen_tri)} triangle, {len(seen_core)} core-number, {len(seen_truss)} truss, {len(seen_gcol)} colouring, {len(seen_msf)} spanning-forest, {len(seen_match)} matching, {len(seen_rcm)} ordering, {len(seen_ilu0)} incomplete-LU, {len(seen_trsv)} triangular-solve and {len(seen_bc)} betweenness kernels checked, {len(bad)} offenders")
sys.exit(1 if bad else 0)
