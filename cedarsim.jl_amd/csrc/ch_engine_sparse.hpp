// ch_engine_sparse.hpp — host side of the sparse path (path 2: blocks too large for LDS): CSR pattern and gather lists, the
// KLU-style plan and its upload, the launches of one LU + solves, and the Newton loop over all samples (kernels: ch_sparse.hpp,
// host analysis: ch_sparse_host.hpp).  Member functions of ch_circuit that own its SparsePath group (sp); they stay
// ch_circuit members because each also needs the description, the sample count or the error text; included by
// ch_engine.hip behind the definition of ch_circuit.
#pragma once

// ------------------------------------------------------------------------------------------
// Sparse path: CSR pattern + gather lists over the global unknown numbering
inline int ch_circuit::build_sparse_structure() {
  hipStream_t st = ctx->stream;
  const int n = desc.A.n_unk, nd = (int)desc.A.edev.size();
  std::vector<std::map<int, std::vector<int>>> rows(n);
  std::vector<std::vector<int>> vrows(n);
  for (int d = 0; d < nd; ++d) {
    const EDev& e = desc.A.edev[d];
    bool vm[NTERM], mm[NTERM * NTERM]; kind_mask(e.kind, vm, mm, e.nt);
    const int stride = desc.A.stride(), gofs = desc.A.g_ofs(), gld = desc.A.g_ld();
    for (int k = 0; k < NTERM; ++k) if (vm[k] && e.term[k] >= 0) vrows[e.term[k]].push_back(d * stride + k);
    for (int k = 0; k < NTERM; ++k) for (int j = 0; j < NTERM; ++j) if (mm[k * NTERM + j] && e.term[k] >= 0 && e.term[j] >= 0) rows[e.term[k]][e.term[j]].push_back(d * stride + gofs + k * gld + j);
  }
  for (int i = 0; i < n; ++i) rows[i][i];  // structural diagonal (gmin stepping, pivots)
  sp.h_rowptr.assign(1, 0); sp.h_colidx.clear();
  std::vector<int> mgp(1, 0), mgs, vgp(1, 0), vgs;
  for (int i = 0; i < n; ++i) {
    for (auto& kv : rows[i]) { sp.h_colidx.push_back(kv.first); mgs.insert(mgs.end(), kv.second.begin(), kv.second.end()); mgp.push_back((int)mgs.size()); }
    sp.h_rowptr.push_back((int)sp.h_colidx.size());
    vgs.insert(vgs.end(), vrows[i].begin(), vrows[i].end()); vgp.push_back((int)vgs.size());
  }
  const size_t nnz = sp.h_colidx.size();
  { std::vector<int> hm, hv;
    for (size_t i = 0; i < nnz; ++i) if (mgp[i + 1] - mgp[i] > SP_ASM_HEAVY) hm.push_back((int)i);
    for (int i = 0; i < n; ++i) if (vgp[i + 1] - vgp[i] > SP_ASM_HEAVY) hv.push_back(i);
    sp.n_heavy_mat = (int)hm.size(); sp.n_heavy_vec = (int)hv.size();
    HIPCHK(sp.heavy_mat.upload(hm, st)); HIPCHK(sp.heavy_vec.upload(hv, st));
    std::vector<int> hr;
    for (int i = 0; i < n; ++i) if (sp.h_rowptr[i + 1] - sp.h_rowptr[i] > 256) hr.push_back(i);
    sp.n_heavy_rows = (int)hr.size();
    HIPCHK(sp.heavy_rows.upload(hr, st)); }
  HIPCHK(sp.rowptr.upload(sp.h_rowptr, st)); HIPCHK(sp.colidx.upload(sp.h_colidx, st)); HIPCHK(sp.mat_gptr.upload(mgp, st)); HIPCHK(sp.mat_gsrc.upload(mgs, st));
  HIPCHK(sp.vec_gptr.upload(vgp, st)); HIPCHK(sp.vec_gsrc.upload(vgs, st));
  HIPCHK(sp.stage.alloc((size_t)tab.S * nd * desc.A.stride())); HIPCHK(sp.Aval.alloc((size_t)tab.S * nnz)); HIPCHK(sp.Cval.alloc((size_t)tab.S * nnz));
  for (DevBuf<double>* b : {&sp.F, &sp.Q, &sp.rhs, &sp.y, &sp.dx, &sp.xcur, &sp.xpred, &sp.hq, &sp.w, &sp.qn}) HIPCHK(b->alloc((size_t)tab.S * n));
  if (sp.h_flag.n < (size_t)tab.S * 2) { HIPCHK(sp.h_red.alloc((size_t)tab.S * 8, hipHostMallocMapped)); HIPCHK(sp.h_flag.alloc((size_t)tab.S * 2, hipHostMallocMapped)); }
  { std::vector<int> z((size_t)tab.S, 0); HIPCHK(sp.dflag.upload(z, st)); }
  sp.rate_v.assign(tab.S, 1.0); sp.status_v.assign(tab.S, 0);
  sp.plan[0].valid = sp.plan[1].valid = false;
  return CH_OK;
}
inline SparseDev ch_circuit::sparse_dev(int which, int sm) {
  SparseDev d; std::memset(&d, 0, sizeof(d));
  SparsePath::PlanDev& pd = sp.plan_dev[which]; const SparsePlan& P = sp.plan[which];
  const size_t n = desc.A.n_unk, nnz = sp.h_colidx.size(), nd = desc.A.edev.size();
  d.rowptr = sp.rowptr.p; d.colidx = sp.colidx.p; d.mat_gptr = sp.mat_gptr.p; d.mat_gsrc = sp.mat_gsrc.p; d.vec_gptr = sp.vec_gptr.p; d.vec_gsrc = sp.vec_gsrc.p;
  d.prow = pd.prow.p; d.pcol = pd.pcol.p; d.a2lu = pd.a2lu.p; d.diag_pos = pd.diag_pos.p; d.lvl_ptr = pd.lvl_ptr.p; d.lvl_rows = pd.lvl_rows.p;
  d.ulvl_ptr = pd.ulvl_ptr.p; d.ulvl_rows = pd.ulvl_rows.p; d.lrow_ptr = pd.lrow_ptr.p; d.l_pos = pd.l_pos.p; d.l_k = pd.l_k.p; d.l_upd_ptr = pd.l_upd_ptr.p;
  d.upd_dst = pd.upd_dst.p; d.upd_src = pd.upd_src.p; d.urow_ptr = pd.urow_ptr.p; d.u_pos = pd.u_pos.p; d.u_col = pd.u_col.p;
  d.lu2a = pd.lu2a.p; d.la_pos = pd.la_pos.p; d.la_diag = pd.la_diag.p; d.lb_dst = pd.lb_dst.p; d.lb_sptr = pd.lb_sptr.p; d.lb_l = pd.lb_l.p; d.lb_u = pd.lb_u.p; d.lb_d = pd.lb_d.p;
  d.fl_rows = pd.fl_rows.p; d.bl_rows = pd.bl_rows.p;
  d.heavy_rows = sp.heavy_rows.p; d.n_heavy_rows = sp.n_heavy_rows;
  d.heavy_mat = sp.heavy_mat.p; d.heavy_vec = sp.heavy_vec.p; d.n_heavy_mat = sp.n_heavy_mat; d.n_heavy_vec = sp.n_heavy_vec;
  d.Lv = pd.Lv.p ? pd.Lv.p + (size_t)sm * (size_t)std::max(0, P.nnz_lu) : nullptr;
  d.s = sm; d.xofs = (long)sm * (long)n;
  d.st_stage = (long)(nd * desc.A.stride()); d.st_nnz = (long)nnz; d.st_lu = (long)std::max(0, P.nnz_lu); d.st_n = (long)n;
  d.stride = desc.A.stride(); d.q_ofs = desc.A.wide ? 8 : 4; d.c_ofs = desc.A.wide ? 64 : 16; d.wide = desc.A.wide ? 1 : 0;
  d.n = desc.A.n_unk; d.nnz = (int)nnz; d.nnz_lu = P.nnz_lu; d.n_lvl = P.valid ? (int)P.lvl_ptr.size() - 1 : 0; d.n_ulvl = P.valid ? (int)P.ulvl_ptr.size() - 1 : 0; d.n_dev = (int)nd;
  // per-sample slices of the work arrays
  d.stage = sp.stage.p + (size_t)sm * nd * desc.A.stride(); d.Aval = sp.Aval.p + (size_t)sm * nnz; d.Cval = sp.Cval.p + (size_t)sm * nnz;
  d.LUv = pd.LUv.p ? pd.LUv.p + (size_t)sm * (size_t)std::max(0, P.nnz_lu) : nullptr;
  d.F = sp.F.p + sm * n; d.Q = sp.Q.p + sm * n; d.rhs = sp.rhs.p + sm * n; d.y = sp.y.p + sm * n; d.dx = sp.dx.p + sm * n;
  d.xcur = sp.xcur.p + sm * n; d.xpred = sp.xpred.p + sm * n; d.hq = sp.hq.p + sm * n; d.w = sp.w.p + sm * n; d.qn = sp.qn.p + sm * n;
  d.red = sp.h_red + (size_t)sm * 8; d.flag = sp.h_flag + (size_t)sm * 2; d.dflag = sp.dflag.p + sm;
  return d;
}
// host analysis from the current numeric values of A (KLU-style: analyse once, refactor many times)
inline int ch_circuit::sparse_plan_from_current(int which, int sm) {
  g_arena = &arena;
  hipStream_t st = ctx->stream;
  std::vector<double> aval(sp.h_colidx.size());
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(aval.data(), sp.Aval.p + (size_t)sm * aval.size(), aval.size() * sizeof(double), hipMemcpyDeviceToHost));
  SparsePlan& P = sp.plan[which];
  int rc = sparse_analyse(desc.A.n_unk, sp.h_rowptr, sp.h_colidx, aval, P);
  if (rc != CH_OK) { set_err("sparse analysis: structurally singular Jacobian"); return rc; }
  SparsePath::PlanDev& pd = sp.plan_dev[which];
  HIPCHK(pd.prow.upload(P.prow, st)); HIPCHK(pd.pcol.upload(P.pcol, st)); HIPCHK(pd.a2lu.upload(P.a2lu, st)); HIPCHK(pd.diag_pos.upload(P.diag_pos, st));
  HIPCHK(pd.lvl_ptr.upload(P.lvl_ptr, st)); HIPCHK(pd.lvl_rows.upload(P.lvl_rows, st)); HIPCHK(pd.ulvl_ptr.upload(P.ulvl_ptr, st)); HIPCHK(pd.ulvl_rows.upload(P.ulvl_rows, st));
  HIPCHK(pd.lrow_ptr.upload(P.lrow_ptr, st)); HIPCHK(pd.l_pos.upload(P.l_pos, st)); HIPCHK(pd.l_k.upload(P.l_k, st)); HIPCHK(pd.l_upd_ptr.upload(P.l_upd_ptr, st));
  HIPCHK(pd.upd_dst.upload(P.upd_dst, st)); HIPCHK(pd.upd_src.upload(P.upd_src, st)); HIPCHK(pd.urow_ptr.upload(P.urow_ptr, st)); HIPCHK(pd.u_pos.upload(P.u_pos, st)); HIPCHK(pd.u_col.upload(P.u_col, st));
  HIPCHK(pd.LUv.alloc((size_t)tab.S * (size_t)P.nnz_lu));
  // subtree form: many independent subtrees under a small separator (ch_sparse_host.hpp SubtreePlan) — three launches per solve
  pd.s3 = P.sub.valid && !env_on(Env::SPARSE_NO_SUBTREE) && !env_on(Env::SPARSE_ONE_WG);
  if (pd.s3) {
    const SubtreePlan& T = P.sub;
    HIPCHK(pd.s3_blob.upload(T.blob, st)); HIPCHK(pd.s3_ptr.upload(T.blob_ptr, st));
    { std::vector<int> ta = T.top_a_idx; if (ta.empty()) ta.push_back(-1); HIPCHK(pd.s3_topa.upload(ta, st)); }
    { std::vector<int> tr = T.top_rows;   // [pivot index | rhs index | dx index] of every top row: one load level in the kernel
      for (int k : T.top_rows) tr.push_back(P.prow[k]);
      for (int k : T.top_rows) tr.push_back(P.pcol[k]);
      if (tr.empty()) tr.push_back(0);
      HIPCHK(pd.s3_topr.upload(tr, st)); }
    HIPCHK(pd.s3_schur.alloc((size_t)tab.S * (size_t)std::max(1, T.nT * T.nT + T.nT) * (size_t)T.n_groups));
    HIPCHK(pd.s3_xT.alloc((size_t)tab.S * (size_t)std::max(1, T.nT)));
    HIPCHK(pd.s3_base.alloc((size_t)tab.S * (size_t)std::max(1, T.nT * T.nT + T.nT)));
    HIPCHK(pd.s3_sum.alloc((size_t)tab.S * (size_t)std::max(1, T.nT * T.nT + T.nT))); HIPCHK(pd.s3_cnt.alloc((size_t)tab.S));
    const int lds3 = T.max_nv * 8 + T.max_blob * 4;
    HIPCHK(hipFuncSetAttribute((const void*)sp3_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, std::max(lds3, 64 * 1024)));
    HIPCHK(hipFuncSetAttribute((const void*)sp3_back_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, std::max(lds3, 64 * 1024)));
    P.wide_levels = false;
    return CH_OK;
  }
  if (P.wide_levels && !env_on(Env::SPARSE_ONE_WG)) {
    std::vector<int> lu2a((size_t)P.nnz_lu, -1);
    for (size_t i = 0; i < P.a2lu.size(); ++i) lu2a[P.a2lu[i]] = (int)i;
    HIPCHK(pd.lu2a.upload(lu2a, st)); HIPCHK(pd.la_pos.upload(P.la_pos, st)); HIPCHK(pd.la_diag.upload(P.la_diag, st));
    HIPCHK(pd.lb_dst.upload(P.lb_dst, st)); HIPCHK(pd.lb_sptr.upload(P.lb_sptr, st)); HIPCHK(pd.lb_l.upload(P.lb_l, st)); HIPCHK(pd.lb_u.upload(P.lb_u, st)); HIPCHK(pd.lb_d.upload(P.lb_d, st));
    HIPCHK(pd.fl_rows.upload(P.fl_rows, st)); HIPCHK(pd.bl_rows.upload(P.bl_rows, st));
    HIPCHK(pd.Lv.alloc((size_t)tab.S * (size_t)P.nnz_lu));
  } else P.wide_levels = false;
  return CH_OK;
}
// refactorisation + both triangular solves for the samples of `wl`: one workgroup per sample (chains, small systems), or
// one launch per elimination level across the whole chip (few wide levels)
inline void ch_circuit::launch_lu_solve(int which, const int* wl, size_t n_work) {
  hipStream_t st = ctx->stream;
  const SparsePlan& P = sp.plan[which];
  const SparseDev d = sparse_dev(which);
  if (sp.plan_dev[which].s3) {
    SparsePath::PlanDev& pd = sp.plan_dev[which]; const SubtreePlan& T = P.sub;
    Sp3Dev q; q.blob = pd.s3_blob.p; q.blob_ptr = pd.s3_ptr.p; q.top_a_idx = pd.s3_topa.p; q.top_rows = pd.s3_topr.p; q.schur = pd.s3_schur.p; q.xT = pd.s3_xT.p; q.top_base = pd.s3_base.p; q.top_sum = pd.s3_sum.p; q.top_cnt = pd.s3_cnt.p;
    q.n_groups = T.n_groups; q.nT = T.nT; q.max_nv = T.max_nv;
    const unsigned lds3 = (unsigned)(T.max_nv * 8 + T.max_blob * 4);
    hipLaunchKernelGGL(sp3_reset_kernel, dim3(1, (unsigned)n_work), dim3(64), 0, st, d, wl, q);
    hipLaunchKernelGGL(sp3_group_kernel, dim3((unsigned)T.n_groups, (unsigned)n_work), dim3(64), lds3, st, d, wl, q);
    hipLaunchKernelGGL(sp3_top_kernel, dim3(SP3_TOP_WG, (unsigned)n_work), dim3(256), 0, st, d, wl, q);
    hipLaunchKernelGGL(sp3_back_kernel, dim3((unsigned)T.n_groups, (unsigned)n_work), dim3(64), lds3, st, d, wl, q);
    stats.n_launch += 4;
    return;
  }
  if (!P.wide_levels) { hipLaunchKernelGGL(sp_lu_solve_kernel, dim3(1, (unsigned)n_work), dim3(1024), 0, st, d, wl); return; }
  const unsigned ny = (unsigned)n_work;
  hipLaunchKernelGGL(sp2_scatter_kernel, dim3((unsigned)((P.nnz_lu + 255) / 256), ny), dim3(256), 0, st, d, wl);
  const int nl = (int)P.lvl_ptr.size() - 1, nul = (int)P.ulvl_ptr.size() - 1;
  for (int l = 0; l < P.n_rlvl; ++l) {
    const int nA = P.la_ptr[l + 1] - P.la_ptr[l], nB = P.lb_ptr[l + 1] - P.lb_ptr[l], nBh = P.lb_nheavy[l], nBl = nB - nBh;
    if (nA + nB == 0) continue;
    const int tb = (nA + nBl + 255) / 256, hb = (nBh + 3) / 4;
    hipLaunchKernelGGL(sp2_factor_level_kernel, dim3((unsigned)std::max(1, tb + hb), ny), dim3(256), 0, st, d, wl, P.la_ptr[l], nA, P.lb_ptr[l], nBl, nBh, tb);
  }
  for (int l = 0; l < nl; ++l) {
    const int nr = P.fl_ptr[l + 1] - P.fl_ptr[l], nh = P.fl_nheavy[l], nlg = nr - nh;
    const int tb = (nlg + 255) / 256, hb = nh;   // one workgroup per heavy row
    hipLaunchKernelGGL(sp2_fwd_level_kernel, dim3((unsigned)std::max(1, tb + hb), ny), dim3(256), 0, st, d, wl, P.fl_ptr[l], nlg, nh, tb);
  }
  for (int l = 0; l < nul; ++l) {
    const int nr = P.bl_ptr[l + 1] - P.bl_ptr[l];
    hipLaunchKernelGGL(sp2_bwd_level_kernel, dim3((unsigned)((nr + 255) / 256), ny), dim3(256), 0, st, d, wl, P.bl_ptr[l], nr);
  }
  stats.n_launch += 1 + P.n_rlvl + nl + nul;
}
// One Newton solve per sample (same contract as the fused kernel: reads the history ring, writes the candidate
// slot).  Samples share the symbolic plan and the pivot order; every phase is queued for all active samples and
// the host synchronises once per phase, so the number of round trips does not grow with the sample count.
// device copies of a sample list / per-sample scales, staged through pinned memory (rewritten only after a stream sync)
inline int ch_circuit::stage_list(int slot, const std::vector<int>& list) {
  if (sp.h_scale.n < (size_t)tab.S) { HIPCHK(sp.h_act.alloc(3 * (size_t)tab.S)); HIPCHK(sp.h_scale.alloc((size_t)tab.S)); }
  g_arena = &arena;
  HIPCHK(sp.act[slot].alloc((size_t)tab.S));
  std::memcpy(sp.h_act + (size_t)slot * tab.S, list.data(), list.size() * sizeof(int));
  HIPCHK(hipMemcpyAsync(sp.act[slot].p, sp.h_act + (size_t)slot * tab.S, list.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  return CH_OK;
}
inline int ch_circuit::run_sparse(NewtonArgs a, const unsigned char* host_active, Summary& out) {
  hipStream_t st = ctx->stream;
  const int which = a.mode == MODE_DC ? 0 : 1;
  const int n = desc.A.n_unk, nd = (int)desc.A.edev.size(), nnz = (int)sp.h_colidx.size();
  // source values always through the device buffer on this path
  if (a.inline_vals) {
    std::memcpy(nwt.h_stage, a.vals_inline, (size_t)(a.nk + a.nsrc) * sizeof(double));
    HIPCHK(hipMemcpyAsync(nwt.d_kv.p, nwt.h_stage, (size_t)(a.nk + a.nsrc) * sizeof(double), hipMemcpyHostToDevice, st));
    a.inline_vals = 0;
  }
  std::memset(&out, 0, sizeof(out));
  const int maxit = a.mode == MODE_EVAL ? 0 : a.maxit;
  std::vector<int> todo;   // samples taking part in this solve
  for (int sm = 0; sm < tab.S; ++sm) {   // a sample takes part when any of its blocks is active (the sparse system spans all blocks)
    bool on = !host_active;
    for (int k = 0; k < desc.A.n_comp && !on; ++k) on = host_active[(size_t)k * tab.S + sm] != 0;
    if (on) todo.push_back(sm);
  }
  if (todo.empty()) return CH_OK;
  std::vector<int> status(tab.S, 1), iters(tab.S, 0);
  std::vector<double> rate_prev(tab.S, 1.0), rate_new(tab.S, -1.0), dn_prev(tab.S, 0.0), fnorm(tab.S, 0.0), scale(tab.S, 1.0);
  for (int sm : todo) rate_prev[sm] = (a.mode == MODE_TRAN && !a.reset_rate) ? sp.rate_v[sm] : 1.0;
  const dim3 b256(256), b1k(1024);
  auto grid = [&](int nx, size_t nl) { return dim3((unsigned)nx, (unsigned)nl); };
  const int gn = (n + 255) / 256, gd = (nd + 63) / 64, ga = (std::max(n, nnz) + 255) / 256;
  // the O(n) passes: one workgroup per sample for small systems, up to SP_NP workgroups + a finishing pass from 4096 rows
  const bool many = n >= 4096;
  const int nbr = std::min(SP_NP, gn);
  g_arena = &arena;
  if (many) { HIPCHK(sp.part.alloc((size_t)tab.S * 8 * SP_NP)); HIPCHK(sp.hrow.alloc((size_t)tab.S * std::max(1, sp.n_heavy_rows) * SP_RB)); }
  if (sp.n_heavy_mat + sp.n_heavy_vec > 0) HIPCHK(sp.hpart.alloc((size_t)tab.S * (sp.n_heavy_mat + sp.n_heavy_vec) * SP_HB * 2));
  // slot 0: every sample of this solve (predict, commit); slot 1: samples still iterating; slot 2: samples to (re)factor
  int rc = stage_list(0, todo); if (rc != CH_OK) return rc;
  hipLaunchKernelGGL(sp_predict_kernel, grid(gn, todo.size()), b256, 0, st, a, sparse_dev(which), (const int*)sp.act[0].p);
  std::vector<int> act = todo;
  rc = stage_list(1, act); if (rc != CH_OK) return rc;
  const bool damp = a.mode == MODE_DC && a.dv_max > 0.0 && (!desc.A.mos_hdev.empty() || desc.A.wide);
  for (int it = 0; it <= maxit && !act.empty(); ++it) {
    {
      const SparseDev d = sparse_dev(which); const int* al = sp.act[1].p;
      hipLaunchKernelGGL(sp_eval_kernel, grid(desc.A.wide ? gd : 2 * gd, act.size()), dim3(64), 0, st, a, d, al);
      hipLaunchKernelGGL(sp_assemble_kernel, grid(ga, act.size()), b256, 0, st, a, d, al);
      if (sp.n_heavy_mat + sp.n_heavy_vec > 0) {
        hipLaunchKernelGGL(sp_assemble_heavy_kernel, grid((sp.n_heavy_mat + sp.n_heavy_vec) * SP_HB, act.size()), b256, 0, st, a, d, al, sp.hpart.p);
        hipLaunchKernelGGL(sp_assemble_heavy_finish_kernel, grid(sp.n_heavy_mat + sp.n_heavy_vec, act.size()), dim3(64), 0, st, a, d, al, (const double*)sp.hpart.p);
      }
      if (a.gshunt != 0.0) hipLaunchKernelGGL(sp_diag_shunt_kernel, grid(gn, act.size()), b256, 0, st, a, d, al);
      if (a.mode == MODE_DC) {
        if (many) { hipLaunchKernelGGL(sp_norms2_kernel, grid(nbr, act.size()), b256, 0, st, a, d, al, 0, sp.part.p, nbr); hipLaunchKernelGGL(sp_finish_kernel, grid(1, act.size()), b256, 0, st, d, al, (const double*)sp.part.p, nbr, 2, (const double*)sp.hrow.p, 0); }
        else hipLaunchKernelGGL(sp_norms_kernel, grid(1, act.size()), b1k, 0, st, a, d, al, 0);
      }
      stats.n_launch += 2;
    }
    if (a.mode == MODE_EVAL) { for (int sm : act) status[sm] = 0; break; }
    if (a.mode == MODE_DC) {
      rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
      std::vector<int> keep;
      for (int sm : act) {
        fnorm[sm] = sp.h_red[(size_t)sm * 8];
        if (!(fnorm[sm] == fnorm[sm]) || fnorm[sm] > 1e300) status[sm] = 2;
        else if (fnorm[sm] < a.dc_abstol) status[sm] = 0;
        else keep.push_back(sm);
      }
      if (keep.size() != act.size()) { act.swap(keep); if (!act.empty()) { rc = stage_list(1, act); if (rc != CH_OK) return rc; } }
      if (act.empty()) break;
    }
    if (it == maxit) break;
    bool fresh = false;
    if (!sp.plan[which].valid) { rc = sparse_plan_from_current(which, act[0]); if (rc != CH_OK) { for (int sm : act) status[sm] = 2; act.clear(); break; } fresh = true; }
    std::vector<int> work = act;   // samples whose factorisation is still to be done in this iteration
    const int* wl = sp.act[1].p;
    for (int attempt = 0; attempt < 2 && !work.empty(); ++attempt) {
      const SparseDev d = sparse_dev(which);
      launch_lu_solve(which, wl, work.size());
      const double* sc = nullptr;
      if (damp) {
        if (many) { hipLaunchKernelGGL(sp_norms2_kernel, grid(nbr, work.size()), b256, 0, st, a, d, wl, 1, sp.part.p, nbr); hipLaunchKernelGGL(sp_finish_kernel, grid(1, work.size()), b256, 0, st, d, wl, (const double*)sp.part.p, nbr, 3, (const double*)sp.hrow.p, 0); }
        else hipLaunchKernelGGL(sp_norms_kernel, grid(1, work.size()), b1k, 0, st, a, d, wl, 1);
        rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
        for (int sm : work) { scale[sm] = 1.0; const double mx = sp.h_red[(size_t)sm * 8 + 1]; if (!sp.h_flag[(size_t)sm * 2] && mx > a.dv_max) scale[sm] = a.dv_max / mx; }
        g_arena = &arena;
        HIPCHK(sp.scale.alloc((size_t)tab.S));
        std::memcpy(sp.h_scale, scale.data(), (size_t)tab.S * sizeof(double));
        HIPCHK(hipMemcpyAsync(sp.scale.p, sp.h_scale, (size_t)tab.S * sizeof(double), hipMemcpyHostToDevice, st));
        sc = sp.scale.p;
      }
      if (many) {   // no-op where the factorisation failed
        hipLaunchKernelGGL(sp_update2_kernel, grid(nbr + sp.n_heavy_rows * SP_RB, work.size()), b256, 0, st, a, d, wl, sc, sp.part.p, nbr, sp.hrow.p);
        hipLaunchKernelGGL(sp_finish_kernel, grid(1, work.size()), b256, 0, st, d, wl, (const double*)sp.part.p, nbr, 0, (const double*)sp.hrow.p, a.mode == MODE_TRAN ? 1 : 0);
      } else hipLaunchKernelGGL(sp_update_kernel, grid(1, work.size()), b1k, 0, st, a, d, wl, sc);
      rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
      stats.n_launch += 2;
      std::vector<int> failed;
      for (int sm : work) if (sp.h_flag[(size_t)sm * 2]) failed.push_back(sm);
      if (failed.empty()) break;
      // a static pivot became zero: re-analyse once with the current values of the first failing sample (KLU would
      // re-pivot here too) and redo the failing samples; the others have already taken their step
      auto drop_failed = [&]() { for (int sm : failed) status[sm] = 2; act.erase(std::remove_if(act.begin(), act.end(), [&](int q) { return status[q] == 2; }), act.end()); };
      if (fresh || attempt == 1) { drop_failed(); work.clear(); break; }
      rc = sparse_plan_from_current(which, failed[0]);
      if (rc != CH_OK) { drop_failed(); break; }
      fresh = true;
      work.swap(failed);
      rc = stage_list(2, work); if (rc != CH_OK) return rc;
      wl = sp.act[2].p;
    }
    std::vector<int> keep;
    for (int sm : act) {
      if (status[sm] == 2) continue;
      ++iters[sm];
      if (sp.h_flag[(size_t)sm * 2 + 1]) { status[sm] = 2; continue; }
      if (a.mode == MODE_TRAN) {
        const double dn = std::sqrt(sp.h_red[(size_t)sm * 8 + 2] / n);
        bool conv = false;
        if (it == 0) conv = dn <= a.newton_tol || (rate_prev[sm] < 0.9 && 2.0 * std::max(rate_prev[sm], 0.02) * dn <= a.newton_tol);
        else { rate_new[sm] = dn_prev[sm] > 0 ? dn / dn_prev[sm] : 0.0; conv = dn <= a.newton_tol; }
        dn_prev[sm] = dn;
        if (conv) { status[sm] = 0; continue; }
      }
      keep.push_back(sm);
    }
    if (keep.size() != act.size()) { act.swap(keep); if (!act.empty()) { rc = stage_list(1, act); if (rc != CH_OK) return rc; } }
  }
  for (int sm : todo) if (a.mode == MODE_TRAN && status[sm] == 0) sp.rate_v[sm] = iters[sm] >= 2 ? std::min(1.0, std::max(rate_new[sm], 1e-4)) : std::min(1.0, rate_prev[sm] * 1.5);
  if (many) {
    hipLaunchKernelGGL(sp_commit2_kernel, grid(nbr, todo.size()), b256, 0, st, a, sparse_dev(which), (const int*)sp.act[0].p, (a.mode == MODE_TRAN) ? 0 : 1, sp.part.p, nbr);
    hipLaunchKernelGGL(sp_finish_kernel, grid(1, todo.size()), b256, 0, st, sparse_dev(which), (const int*)sp.act[0].p, (const double*)sp.part.p, nbr, 1, (const double*)sp.hrow.p, 0);
  } else hipLaunchKernelGGL(sp_commit_kernel, grid(1, todo.size()), b1k, 0, st, a, sparse_dev(which), (const int*)sp.act[0].p, (a.mode == MODE_TRAN) ? 0 : 1);
  rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
  stats.n_launch += 1;
  for (int sm : todo) {
    sp.status_v[sm] = status[sm];
    if (status[sm] != 0) ++out.n_fail;
    if (status[sm] == 2) ++out.n_singular;
    out.max_iters = std::max(out.max_iters, iters[sm]); out.sum_iters += iters[sm]; out.sum_block_iters += iters[sm]; out.fnorm = std::max(out.fnorm, fnorm[sm]);
    const double* r = sp.h_red + (size_t)sm * 8;
    if (a.mode == MODE_TRAN && r[7] > 0) {
      out.errk = std::max(out.errk, a.ck * std::sqrt(r[4] / r[7])); out.errkm1 = std::max(out.errkm1, a.ckm1 * std::sqrt(r[5] / r[7])); out.errkp1 = std::max(out.errkp1, a.ckp1 * std::sqrt(r[6] / r[7]));
    }
  }
  return CH_OK;
}
