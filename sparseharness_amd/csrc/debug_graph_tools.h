// debug_graph_tools.h -- the tools build only (SH_PLAN_EMULATE), included behind the graph handles of engine.hip.
// Graph and worklist hygiene (tests/test_graph_hygiene_gpu.py): what a call reads of its handle is what the handle was
// built with or what the call wrote itself.  sh_debug_poison_graph drains the stream, then fills every array of the handle
// that a call reads only after writing it, as sh_debug_poison_scratch does for a matrix.  The rule for the word:
//   - a data word (control block and the per-workgroup parts, minima and picks behind it, bitmaps, stamps, remaining
//     degrees, supports) gets data_word;
//   - a word that is used as an index (a vertex or edge id of a queue or work list) gets index_word, which the caller
//     chooses as a VALID id whose consumption would change the answer; a piece record gets {index_word, 0}, the first
//     piece of that vertex's list;
//   - arrays built once (d_in_*, d_out_*, weights, d_rpieces, d_deg, d_eid, d_eu, d_ev, d_wk, d_S, the forward lists and
//     the control block of sh_tri_graph) are not touched.
// So a call that consumes a poisoned word gives a wrong answer, not a wild access.  index_word is checked against the
// handle (rows; edges for sh_truss_graph; min(rows, edges) for sh_msf_graph and sh_match_graph, whose parent words hold
// vertices and whose work lists hold edges) before anything is filled.
// kind: 0 sh_frontier, 1 sh_bfs_graph, 2 sh_sssp_graph, 3 sh_scc_graph, 4 sh_wcc_graph, 5 sh_tri_graph, 6 sh_core_graph,
// 7 sh_truss_graph, 8 sh_color_graph, 9 sh_msf_graph, 10 sh_match_graph, 11 sh_rcm_graph (the order of the header).
// What is left out of a handle, and why, is listed case by case below and in DESIGN.md "Graph and worklist hygiene".
// sizes[0..SH_DEBUG_GRAPH_SIZES): the bytes filled per array, in the order of the `fill` calls below; the rest 0.
#pragma once

constexpr int SH_DEBUG_GRAPH_SIZES = 12;

extern "C" int sh_debug_poison_graph(sh_engine *e, int kind, void *handle, uint32_t data_word, uint32_t index_word, int64_t *sizes) {
  if (!e || !handle || !sizes) return SH_EINVAL;
  if (hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return SH_EHIP;
  for (int i = 0; i < SH_DEBUG_GRAPH_SIZES; i++) sizes[i] = 0;
  bool ok = true;
  int at = 0;
  const DevArrays *dev = nullptr;
  auto fill = [&](void *p, uint32_t word) {   // the whole array behind p, as the handle allocated it
    const size_t bytes = p ? dev->size_of(p) : 0;
    if (bytes >= 4) ok = ok && hipMemsetD32Async((hipDeviceptr_t)p, (int)word, bytes / 4, e->stream) == hipSuccess;
    sizes[at++] = (int64_t)(bytes / 4 * 4);
  };
  auto fill_pieces = [&](WlPiece *p) {   // {index_word, 0} throughout
    const size_t n = p ? dev->size_of(p) / sizeof(WlPiece) : 0;
    if (n > 0) {
      const std::vector<WlPiece> host(n, WlPiece{index_word, 0u});
      ok = ok && hipMemcpy(p, host.data(), n * sizeof(WlPiece), hipMemcpyHostToDevice) == hipSuccess;
    }
    sizes[at++] = (int64_t)(n * sizeof(WlPiece));
  };
  auto fill_picks = [&](SccPick *p, size_t n) {   // a candidate record holds a vertex: {data_word twice, index_word, data_word}
    const std::vector<SccPick> host(n, SccPick{((uint64_t)data_word << 32) | data_word, (int32_t)index_word, (int32_t)data_word});
    ok = ok && hipMemcpy(p, host.data(), n * sizeof(SccPick), hipMemcpyHostToDevice) == hipSuccess;
    sizes[at++] = (int64_t)(n * sizeof(SccPick));
  };
  switch (kind) {
    case 0: {
      // d_stamp is NOT per call: it holds the number of the sparse launch that claimed a row last, sh_frontier::gen goes on
      // counting from call to call, and the stamps are cleared at creation and when gen wraps only (launch_sparse).  A
      // poisoned stamp equal to a later gen would be state the handle never had.  d_row_ptr / d_col / d_val, d_col_ptr and
      // d_row_of are built once.
      sh_frontier *f = (sh_frontier *)handle;
      if ((int64_t)index_word >= f->rows) return SH_EINVAL;
      dev = &f->dev;
      fill(f->d_ctl, data_word);     // FrontierCtl
      fill(f->d_side, data_word);    // the raw reductions of the active rows
      fill(f->d_clist, index_word);  // rows
      fill(f->d_alist, index_word);  // rows; a piece of d_rplist names a slot of this list, and rows slots there are
      fill_pieces(f->d_cplist);
      fill_pieces(f->d_rplist);
      break;
    }
    case 1: {
      sh_bfs_graph *g = (sh_bfs_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);   // BfsCtl and the WlParts
      for (int i = 0; i < 2; i++) fill(g->d_bm[i], data_word);
      for (int i = 0; i < 2; i++) fill(g->d_queue[i], index_word);
      for (int i = 0; i < 2; i++) fill_pieces(g->d_opieces[i]);
      break;
    }
    case 2: {
      sh_sssp_graph *g = (sh_sssp_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);   // SsspCtl, the WlParts and the split's minima (d_pmin)
      fill(g->d_stamp, data_word);
      for (int i = 0; i < 2; i++) fill(g->d_near[i], index_word);
      for (int i = 0; i < 2; i++) fill(g->d_far[i], index_word);
      for (int i = 0; i < 2; i++) fill_pieces(g->d_opieces[i]);
      break;
    }
    case 3: {
      // d_colour holds vertex ids and gets data_word all the same: no kernel of scc.hip.h indexes by a colour, it is
      // compared (scc_propagate, scc_claim, scc_label) and stored into comp as a label (scc_claim).
      sh_scc_graph *g = (sh_scc_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      ok = ok && hipMemsetD32Async((hipDeviceptr_t)g->d_ctl, (int)data_word, (SCC_CTL_BYTES + SCC_PART_BYTES) / 4, e->stream) == hipSuccess;
      sizes[at++] = SCC_CTL_BYTES + SCC_PART_BYTES;   // SccCtl and the WlParts
      fill_picks(g->d_pick, SCC_MAX_BLOCKS);
      fill(g->d_colour, data_word);
      fill(g->d_stamp, data_word);
      fill(g->d_cand, index_word);
      for (int i = 0; i < 2; i++) fill(g->d_list[i], index_word);
      for (int i = 0; i < 2; i++) fill_pieces(g->d_opieces[i]);
      for (int i = 0; i < 2; i++) fill_pieces(g->d_ipieces[i]);
      break;
    }
    case 4: {
      sh_wcc_graph *g = (sh_wcc_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);       // WccCtl, the WlParts of the walk and those of the jumps (d_jpart)
      fill(g->d_parent, index_word);   // p[v]: wcc_hook and wcc_jump index by it
      fill(g->d_list, index_word);
      fill_pieces(g->d_ipieces);
      fill_pieces(g->d_opieces);
      break;
    }
    case 5: {   // (the TriCtl in front of the parts is built once)
      sh_tri_graph *g = (sh_tri_graph *)handle;
      if (g->d_part) {
        ok = ok && hipMemsetD32Async((hipDeviceptr_t)g->d_part, (int)data_word, 2 * TRI_PART_BYTES / 4, e->stream) == hipSuccess;
        sizes[at++] = 2 * TRI_PART_BYTES;
      }
      break;
    }
    case 6: {
      sh_core_graph *g = (sh_core_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);   // CoreCtl, the WlParts and the minima (d_mins)
      fill(g->d_cur, data_word);
      for (int i = 0; i < 2; i++) fill(g->lists.list[i], index_word);
      for (int i = 0; i < 2; i++) fill_pieces(g->lists.pieces[i]);
      break;
    }
    case 7: {
      sh_truss_graph *g = (sh_truss_graph *)handle;
      if ((int64_t)index_word >= g->edges) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);   // TrussCtl, the parts of the peel, the minima (d_mins) and the parts of the support pass (d_sparts)
      fill(g->d_sup, data_word);
      fill(g->d_stamp, data_word);
      for (int i = 0; i < 2; i++) fill(g->lists.list[i], index_word);
      break;
    }
    case 8: {
      // d_deg and the symmetric lists (d_in_ptr, d_in_col) are built once.  d_wait is zeroed for every row by gcol_init,
      // the WlParts are written by every workgroup of gcol_assign before gcol_close sums them, and a work list is read
      // up to the counts of the control block only, which sh_color zeroes.
      sh_color_graph *g = (sh_color_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);   // ColorCtl and the WlParts
      fill(g->d_wait, data_word);
      for (int i = 0; i < 2; i++) fill(g->lists.list[i], index_word);   // vertices
      break;
    }
    case 9: {
      // d_eu, d_ev and d_wk are built once.  msf_init writes p, best and list 0 whole; to[r] is written by msf_pick for
      // exactly the roots whose word msf_link reads; the WlParts of msf_link and of the jumps (d_jpart, behind them in
      // d_ctl's allocation) are written by every workgroup of a round before msf_close sums them.  p and to hold vertex
      // ids and the lists edge ids: index_word has to be valid as both.
      sh_msf_graph *g = (sh_msf_graph *)handle;
      if ((int64_t)index_word >= std::min(g->rows, g->edges)) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);    // MsfCtl, the WlParts of msf_link and those of the jumps (d_jpart)
      fill(g->d_best, data_word);   // (64-bit words: data_word twice; 0 is a key below every bid)
      fill(g->d_p, index_word);     // vertices: msf_find, msf_pick and msf_jump index by it
      fill(g->d_to, index_word);    // vertices: msf_link stores it into p
      for (int i = 0; i < 2; i++) fill(g->lists.list[i], index_word);   // edges
      break;
    }
    case 10: {
      // d_eu, d_ev and d_wk are built once (build_weighted_edges, as for sh_msf_graph); mate is the caller's vector.
      // match_init writes best and list 0 whole, match_bid fills the other list up to the count match_take and
      // match_clear read, and every workgroup of match_take writes its WlPart before match_close sums them.  The handle
      // has no array of vertex ids; index_word is checked as for sh_msf_graph all the same, so that one word serves both.
      sh_match_graph *g = (sh_match_graph *)handle;
      if ((int64_t)index_word >= std::min(g->rows, g->edges)) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);    // MatchCtl and the WlParts
      fill(g->d_best, data_word);   // (64-bit words: data_word twice; 0 is a key below every bid)
      for (int i = 0; i < 2; i++) fill(g->lists.list[i], index_word);   // edges
      break;
    }
    case 11: {
      // d_S, d_in_ptr and d_in_col (the lists over the labels) are built once.  rcm_init writes posl, levl, stamp and
      // owner whole in every call; cnt[i] is written by rcm_count for the positions rcm_place reads; order is read in
      // [a, b) and below `done` only, which the call wrote; the WlParts are written by every workgroup of rcm_sweep or
      // rcm_count before they are read, the RcmFins (d_fin, behind them in d_ctl's allocation) by rcm_finish before
      // rcm_total.  Only order is used as an index (labels); posl, levl, stamp, owner and cnt are compared or stored.
      sh_rcm_graph *g = (sh_rcm_graph *)handle;
      if ((int64_t)index_word >= g->rows) return SH_EINVAL;
      dev = &g->dev;
      fill(g->d_ctl, data_word);   // RcmCtl, the WlParts and the RcmFins (d_fin)
      fill(g->st.order, index_word);
      fill(g->st.posl, data_word);
      fill(g->st.levl, data_word);
      fill(g->st.stamp, data_word);
      fill(g->st.owner, data_word);
      fill(g->st.cnt, data_word);
      break;
    }
    default:
      return SH_EINVAL;
  }
  return ok && hipStreamSynchronize(e->stream) == hipSuccess ? SH_OK : SH_EHIP;
}
