// ch_engine_sparse.hpp — host side of the sparse path (path 2: blocks too large for LDS).  Kernels: ch_sparse.hpp; host analysis
// (the KLU-style plan) and its row-wise replay: ch_sparse_host.hpp; the per-sample Newton decisions: ch_sparse_newton.hpp (both
// HIP-free, tested on the CPU).  What is left here owns the stream:
//   build_sparse_structure    CSR pattern, gather lists, work arrays, grid sizes — once per circuit and sample count
//   sparse_plan_from_current  analysis from the current values of A, upload of the plan: one loop over SP_PLAN_ARRAYS (ch_sparse.hpp),
//                             the one list of the plan's index arrays; the subtree form's buffers, kernel arguments and LDS size
//   sparse_dev                the kernels' argument struct: the same loop + the scalars and the per-sample slices of the work arrays
//   sp_launch_*               one launcher per pass (residual = eval + assembly, norms, LU + solves, update, commit); each hides the
//                             choice between the one-workgroup kernel of small systems and the two-stage kernels from 4096 rows
//   run_sparse                one Newton solve for all samples: predict -> { residual -> [DC test] -> factor + step, one retry
//                             (sp_factor_and_step) -> convergence } -> commit -> summary; stages the sample lists, waits once per
//                             phase and hands the mapped numbers to sp.newton, which decides
// Member functions of ch_circuit that own its SparsePath group (sp); they stay ch_circuit members because each also needs the
// description, the sample count or the error text; included by ch_engine.hip behind the definition of ch_circuit.
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
  sp.grid.gn = (n + 255) / 256; sp.grid.gd = (nd + 63) / 64; sp.grid.ga = (std::max(n, (int)nnz) + 255) / 256;
  sp.grid.many = n >= 4096; sp.grid.nbr = std::min(SP_NP, sp.grid.gn);
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
  sp.newton.reset(tab.S);
  sp.plan[0].valid = sp.plan[1].valid = false;
  return CH_OK;
}
inline SparseDev ch_circuit::sparse_dev(int which, int sm) {
  SparseDev d; std::memset(&d, 0, sizeof(d));
  SparsePath::PlanDev& pd = sp.plan_dev[which]; const SparsePlan& P = sp.plan[which];
  const size_t n = desc.A.n_unk, nnz = sp.h_colidx.size(), nd = desc.A.edev.size();
  d.rowptr = sp.rowptr.p; d.colidx = sp.colidx.p; d.mat_gptr = sp.mat_gptr.p; d.mat_gsrc = sp.mat_gsrc.p; d.vec_gptr = sp.vec_gptr.p; d.vec_gsrc = sp.vec_gsrc.p;
  for (int i = 0; i < SP_N_PLAN_ARRAYS; ++i) d.*SP_PLAN_ARRAYS[i].dev = pd.idx[i].p;
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
  for (int i = 0; i < SP_N_PLAN_ARRAYS; ++i) if (!SP_PLAN_ARRAYS[i].level_form) HIPCHK(pd.idx[i].upload(P.*SP_PLAN_ARRAYS[i].host, st));
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
    Sp3Dev& q = pd.s3_dev;   // the buffers keep their addresses until the next analysis
    q.blob = pd.s3_blob.p; q.blob_ptr = pd.s3_ptr.p; q.top_a_idx = pd.s3_topa.p; q.top_rows = pd.s3_topr.p; q.schur = pd.s3_schur.p; q.xT = pd.s3_xT.p; q.top_base = pd.s3_base.p; q.top_sum = pd.s3_sum.p; q.top_cnt = pd.s3_cnt.p;
    q.n_groups = T.n_groups; q.nT = T.nT; q.max_nv = T.max_nv;
    pd.s3_lds = (unsigned)(T.max_nv * 8 + T.max_blob * 4);   // a group's wavefront: its values + its blob
    HIPCHK(hipFuncSetAttribute((const void*)sp3_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, std::max((int)pd.s3_lds, 64 * 1024)));
    HIPCHK(hipFuncSetAttribute((const void*)sp3_back_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, std::max((int)pd.s3_lds, 64 * 1024)));
    P.wide_levels = false;
    return CH_OK;
  }
  if (P.wide_levels && !env_on(Env::SPARSE_ONE_WG)) {
    for (int i = 0; i < SP_N_PLAN_ARRAYS; ++i) if (SP_PLAN_ARRAYS[i].level_form) HIPCHK(pd.idx[i].upload(P.*SP_PLAN_ARRAYS[i].host, st));
    HIPCHK(pd.Lv.alloc((size_t)tab.S * (size_t)P.nnz_lu));
  } else P.wide_levels = false;
  return CH_OK;
}
// device copies of a sample list, staged through pinned memory (rewritten only after a stream sync).  Slot 0: every sample of this
// solve (predict, commit); slot 1: samples still iterating; slot 2: samples to factor again
inline int ch_circuit::stage_list(int slot, const std::vector<int>& list) {
  if (sp.h_scale.n < (size_t)tab.S) { HIPCHK(sp.h_act.alloc(3 * (size_t)tab.S)); HIPCHK(sp.h_scale.alloc((size_t)tab.S)); }
  g_arena = &arena;
  HIPCHK(sp.act[slot].alloc((size_t)tab.S));
  std::memcpy(sp.h_act + (size_t)slot * tab.S, list.data(), list.size() * sizeof(int));
  HIPCHK(hipMemcpyAsync(sp.act[slot].p, sp.h_act + (size_t)slot * tab.S, list.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  return CH_OK;
}

// ------------------------------------------------------------------------------------------
// The launchers: every kernel of this path takes all samples of `list` in one launch (blockIdx.y walks the list).
// stats.n_launch counts fewer launches than this path issues: 2 per residual pass whatever it launches, 2 per update (the norms
// and finishing passes ride along), 1 per commit, nothing for the predictor and the one-workgroup LU.  ch_stats has always shown
// these figures and the recorded traces compare them: they stay as they are.
static inline dim3 sp_grid(int nx, size_t n_list) { return dim3((unsigned)nx, (unsigned)n_list); }
// device evaluation and assembly of A = G + alpha0 C, C, F, Q (the heavy gather items in slices, the diagonal shunt of gmin
// stepping); at the operating point also the residual norm
inline void ch_circuit::sp_launch_residual(const NewtonArgs& a, const SparseDev& d, const int* list, size_t count) {
  hipStream_t st = ctx->stream; const SpGrids& g = sp.grid; const int n_heavy = sp.n_heavy_mat + sp.n_heavy_vec;
  hipLaunchKernelGGL(sp_eval_kernel, sp_grid(desc.A.wide ? g.gd : 2 * g.gd, count), dim3(64), 0, st, a, d, list);
  hipLaunchKernelGGL(sp_assemble_kernel, sp_grid(g.ga, count), dim3(256), 0, st, a, d, list);
  if (n_heavy > 0) {
    hipLaunchKernelGGL(sp_assemble_heavy_kernel, sp_grid(n_heavy * SP_HB, count), dim3(256), 0, st, a, d, list, sp.hpart.p);
    hipLaunchKernelGGL(sp_assemble_heavy_finish_kernel, sp_grid(n_heavy, count), dim3(64), 0, st, a, d, list, (const double*)sp.hpart.p);
  }
  if (a.gshunt != 0.0) hipLaunchKernelGGL(sp_diag_shunt_kernel, sp_grid(g.gn, count), dim3(256), 0, st, a, d, list);
  if (a.mode == MODE_DC) sp_launch_norms(a, d, 0, list, count);
  stats.n_launch += 2;
}
// what = 0: max |F| -> red[0]; what = 1: max |dx| -> red[1]
inline void ch_circuit::sp_launch_norms(const NewtonArgs& a, const SparseDev& d, int what, const int* list, size_t count) {
  hipStream_t st = ctx->stream; const SpGrids& g = sp.grid;
  if (g.many) {
    hipLaunchKernelGGL(sp_norms2_kernel, sp_grid(g.nbr, count), dim3(256), 0, st, a, d, list, what, sp.part.p, g.nbr);
    hipLaunchKernelGGL(sp_finish_kernel, sp_grid(1, count), dim3(256), 0, st, d, list, (const double*)sp.part.p, g.nbr, 2 + what, (const double*)sp.hrow.p, 0);
  } else hipLaunchKernelGGL(sp_norms_kernel, sp_grid(1, count), dim3(1024), 0, st, a, d, list, what);
}
// refactorisation + both triangular solves: the subtree form (three launches + a reset), one workgroup per sample (chains, small
// systems), or one launch per elimination level across the whole chip (few wide levels)
inline void ch_circuit::sp_launch_lu_solve(int which, const SparseDev& d, const int* wl, size_t n_work) {
  hipStream_t st = ctx->stream;
  const SparsePlan& P = sp.plan[which]; const SparsePath::PlanDev& pd = sp.plan_dev[which];
  const unsigned ny = (unsigned)n_work;
  if (pd.s3) {
    const Sp3Dev& q = pd.s3_dev; const unsigned ng = (unsigned)P.sub.n_groups;
    hipLaunchKernelGGL(sp3_reset_kernel, dim3(1, ny), dim3(64), 0, st, d, wl, q);
    hipLaunchKernelGGL(sp3_group_kernel, dim3(ng, ny), dim3(64), pd.s3_lds, st, d, wl, q);
    hipLaunchKernelGGL(sp3_top_kernel, dim3(SP3_TOP_WG, ny), dim3(256), 0, st, d, wl, q);
    hipLaunchKernelGGL(sp3_back_kernel, dim3(ng, ny), dim3(64), pd.s3_lds, st, d, wl, q);
    stats.n_launch += 4;
    return;
  }
  if (!P.wide_levels) { hipLaunchKernelGGL(sp_lu_solve_kernel, dim3(1, ny), dim3(1024), 0, st, d, wl); return; }
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
// x += scale * dx, charge, sum (w dx)^2 -> red[2], non-finite -> flag[1]; a no-op where the factorisation failed
inline void ch_circuit::sp_launch_update(const NewtonArgs& a, const SparseDev& d, const int* list, size_t count, const double* scale) {
  hipStream_t st = ctx->stream; const SpGrids& g = sp.grid;
  if (g.many) {
    hipLaunchKernelGGL(sp_update2_kernel, sp_grid(g.nbr + sp.n_heavy_rows * SP_RB, count), dim3(256), 0, st, a, d, list, scale, sp.part.p, g.nbr, sp.hrow.p);
    hipLaunchKernelGGL(sp_finish_kernel, sp_grid(1, count), dim3(256), 0, st, d, list, (const double*)sp.part.p, g.nbr, 0, (const double*)sp.hrow.p, a.mode == MODE_TRAN ? 1 : 0);
  } else hipLaunchKernelGGL(sp_update_kernel, sp_grid(1, count), dim3(1024), 0, st, a, d, list, scale);
}
// candidate state and charge into the ring, local-error sums -> red[4..7]
inline void ch_circuit::sp_launch_commit(const NewtonArgs& a, const SparseDev& d, const int* list, size_t count) {
  hipStream_t st = ctx->stream; const SpGrids& g = sp.grid; const int dc = (a.mode == MODE_TRAN) ? 0 : 1;
  if (g.many) {
    hipLaunchKernelGGL(sp_commit2_kernel, sp_grid(g.nbr, count), dim3(256), 0, st, a, d, list, dc, sp.part.p, g.nbr);
    hipLaunchKernelGGL(sp_finish_kernel, sp_grid(1, count), dim3(256), 0, st, d, list, (const double*)sp.part.p, g.nbr, 1, (const double*)sp.hrow.p, 0);
  } else hipLaunchKernelGGL(sp_commit_kernel, sp_grid(1, count), dim3(1024), 0, st, a, d, list, dc);
}

// ------------------------------------------------------------------------------------------
// Factorisation + Newton step of the samples still iterating (list slot 1), with ONE retry: where a static pivot became zero the
// plan is made again from the current values of the first failing sample and the failing samples (list slot 2) are done again;
// the others have already taken their step.  fresh: the plan was made in this iteration; damp: uniform voltage limiting.
inline int ch_circuit::sp_factor_and_step(const NewtonArgs& a, int which, bool fresh, bool damp) {
  SparseNewton& nw = sp.newton;
  nw.begin_factor();
  const int* wl = sp.act[1].p;
  for (int attempt = 0; attempt < 2 && !nw.work.empty(); ++attempt) {
    const SparseDev d = sparse_dev(which);
    const size_t count = nw.work.size();
    sp_launch_lu_solve(which, d, wl, count);
    const double* sc = nullptr;
    if (damp) {
      sp_launch_norms(a, d, 1, wl, count);
      int rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
      nw.limit_steps(sp.h_red, sp.h_flag);
      g_arena = &arena;
      HIPCHK(sp.scale.alloc((size_t)tab.S));
      std::memcpy(sp.h_scale, nw.scale.data(), (size_t)tab.S * sizeof(double));
      HIPCHK(hipMemcpyAsync(sp.scale.p, sp.h_scale, (size_t)tab.S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      sc = sp.scale.p;
    }
    sp_launch_update(a, d, wl, count, sc);
    int rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
    stats.n_launch += 2;
    if (nw.after_factor(sp.h_flag, fresh, attempt) != SparseNewton::Factored::REANALYSE) break;   // done, or the failing samples dropped as singular
    rc = sparse_plan_from_current(which, nw.failed[0]);
    if (rc != CH_OK) { nw.drop_failed(); break; }
    fresh = true;
    nw.retry_failed();
    rc = stage_list(2, nw.work); if (rc != CH_OK) return rc;
    wl = sp.act[2].p;
  }
  return CH_OK;
}
// One Newton solve per sample (same contract as the fused kernel: reads the history ring, writes the candidate slot).  Samples
// share the symbolic plan and the pivot order; every phase is queued for all active samples and the host synchronises once per
// phase, so the number of round trips does not grow with the sample count.  Every decision is sp.newton's.
inline int ch_circuit::run_sparse(NewtonArgs a, const unsigned char* host_active, Summary& out) {
  hipStream_t st = ctx->stream;
  const int which = a.mode == MODE_DC ? 0 : 1;
  SparseNewton& nw = sp.newton; const SpGrids& g = sp.grid;
  // source values always through the device buffer on this path
  if (a.inline_vals) {
    std::memcpy(nwt.h_stage, a.vals_inline, (size_t)(a.nk + a.nsrc) * sizeof(double));
    HIPCHK(hipMemcpyAsync(nwt.d_kv.p, nwt.h_stage, (size_t)(a.nk + a.nsrc) * sizeof(double), hipMemcpyHostToDevice, st));
    a.inline_vals = 0;
  }
  std::memset(&out, 0, sizeof(out));
  const int maxit = a.mode == MODE_EVAL ? 0 : a.maxit;
  SparseNewton::Solve cfg;
  cfg.dc = a.mode == MODE_DC; cfg.tran = a.mode == MODE_TRAN; cfg.reset_rate = a.reset_rate != 0; cfg.n = desc.A.n_unk;
  cfg.newton_tol = a.newton_tol; cfg.dc_abstol = a.dc_abstol; cfg.dv_max = a.dv_max;
  nw.begin(cfg, host_active, desc.A.n_comp);
  if (nw.todo.empty()) return CH_OK;
  g_arena = &arena;
  if (g.many) { HIPCHK(sp.part.alloc((size_t)tab.S * 8 * SP_NP)); HIPCHK(sp.hrow.alloc((size_t)tab.S * std::max(1, sp.n_heavy_rows) * SP_RB)); }
  if (sp.n_heavy_mat + sp.n_heavy_vec > 0) HIPCHK(sp.hpart.alloc((size_t)tab.S * (sp.n_heavy_mat + sp.n_heavy_vec) * SP_HB * 2));
  // ---- predict ----
  int rc = stage_list(0, nw.todo); if (rc != CH_OK) return rc;
  const int* all = sp.act[0].p;
  hipLaunchKernelGGL(sp_predict_kernel, sp_grid(g.gn, nw.todo.size()), dim3(256), 0, st, a, sparse_dev(which), all);
  rc = stage_list(1, nw.act); if (rc != CH_OK) return rc;
  const bool damp = a.mode == MODE_DC && a.dv_max > 0.0 && (!desc.A.mos_hdev.empty() || desc.A.wide);
  for (int it = 0; it <= maxit && !nw.act.empty(); ++it) {
    // ---- residual ----
    sp_launch_residual(a, sparse_dev(which), sp.act[1].p, nw.act.size());
    if (a.mode == MODE_EVAL) { nw.accept_all(); break; }
    if (a.mode == MODE_DC) {
      rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
      if (nw.dc_residual(sp.h_red) && !nw.act.empty()) { rc = stage_list(1, nw.act); if (rc != CH_OK) return rc; }
      if (nw.act.empty()) break;
    }
    if (it == maxit) break;
    // ---- factor + step ----
    bool fresh = false;
    if (!sp.plan[which].valid) { rc = sparse_plan_from_current(which, nw.act[0]); if (rc != CH_OK) { nw.drop_all_singular(); break; } fresh = true; }
    rc = sp_factor_and_step(a, which, fresh, damp); if (rc != CH_OK) return rc;
    // ---- convergence ----
    if (nw.after_update(it, sp.h_red, sp.h_flag) && !nw.act.empty()) { rc = stage_list(1, nw.act); if (rc != CH_OK) return rc; }
  }
  nw.end_iterations();
  // ---- commit, summary ----
  sp_launch_commit(a, sparse_dev(which), all, nw.todo.size());
  rc = poll_stream("sparse path: "); if (rc != CH_OK) return rc;
  stats.n_launch += 1;
  nw.summarise(out, sp.h_red, a.ck, a.ckm1, a.ckp1);
  return CH_OK;
}
