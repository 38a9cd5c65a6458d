// ch_engine_transens.hpp — transient parameter sensitivities by the direct method (ch_tran_sens): the host stepper's transient, state
// path untouched, plus at every accepted step one unperturbed MODE_EVAL launch (G, C, f, q at the accepted state), one or two perturbed
// ones per parameter, and transens_step_kernel (ch_transens_kernels.hpp): one step of the s / w recursion of ch_transens_host.hpp for
// all parameters.  Steps, divisors and perturbed values come from the step plan of ch_dc_sens (SensPlan, ch_sens_host.hpp).  The
// perturbed tables of every (parameter, sign) are built and uploaded ONCE per transient into buffers of their
// own (TranSensSet); the loop only points NewtonArgs at them and evaluates the (host-side) perturbed source tables at each step's
// source time.  The evaluations read the accepted ring slot and send their candidate row to the slot that is free between attempts;
// they write neither the convergence rates nor the pivot orders, so the next attempt starts from what ch_tran would have.
// Included by ch_engine.hip behind ch_engine_sens.hpp.
#pragma once

extern "C++" {   // (included inside the extern "C" block of ch_engine.hip)

// the tables of one (parameter, sign), built once per transient
struct TranSensSet {
  Sensitivity store;       // device copies (own allocations: freed with the set)
  TableOverride o;         // host copies; the source tables are read at every step
  NewtonArgs a;            // the circuit's argument template pointed at the copies
  size_t lds_extra = 0;
};

struct TranSens {
  int n_par = 0, S = 0, nblk = 0, ds = 0, nu = 0, n_obs = 0, kc = 1, bchunk = 1; size_t nA = 0, nF = 0;
  const ch_tran_opts* o = nullptr;
  SensPlan plan;                                             // the step plan of ch_dc_sens (ch_sens_host.hpp)
  std::vector<char> is_value;                                // per parameter: the slot IS the value of a DC source
  std::vector<std::unique_ptr<TranSensSet>> plus, minus;     // minus[k] is null for a forward difference
  DevBuf<double> d_S, d_W, d_Fp, d_Fm, d_Qp, d_Qm, d_Q0, d_den; DevBuf<int> d_central, d_fail;
  ScopedWorkspace work;                                      // above 96 unknowns: the global workspace of transens_step_kernel<256>
  const BlockMeta* bmeta = nullptr;
  RowStore rows;
  long n_eval = 0, n_solve_launches = 0, n_points = 0, n_solved = 0, n_factor_chunks = 0;   // points; of them solved; their chunks
  double build_s = 0, eval_s = 0; float eval_ms = 0, solve_ms = 0; bool profile = false;
};
struct TranSensScope { ch_circuit* c; TranSensScope(ch_circuit* c_, TranSens* t) : c(c_) { c->tsens = t; } ~TranSensScope() { c->tsens = nullptr; } };

static const char* transens_src_field(const HSource& s, int b) {
  static const char* const pulse[] = {"v1", "v2", "td", "tr", "tf", "pw", "period"};
  static const char* const sine[] = {"vo", "va", "freq", "td", "theta", "phase", "ncycles"};
  if (s.kind == CH_SRC_PULSE && b >= 0 && b < 7) return pulse[b];
  if (s.kind == CH_SRC_SIN && b >= 0 && b < 7) return sine[b];
  return "value";
}

// the step plan of the call; a slot that moves a break point is refused here, before any launch
static int transens_steps(ch_circuit* c, TranSens& T, const int32_t* slot_ids, const ch_sens_opts& sopt, double t0, double t1) {
  T.plan = sens_plan_of(c, T.n_par, slot_ids, sopt);
  const SensPlan& P = T.plan;
  T.is_value.assign(T.n_par, 0);
  for (int k = 0; k < T.n_par; ++k) {
    if (!P.is_src(k)) continue;
    const int id = P.slot[k], sa = P.src_of[k];
    T.is_value[k] = P.kind[k] == CH_SLOT_SRC_DC && c->desc.src[sa].kind == CH_SRC_DC;
    for (int sign = +1; sign >= (P.central[k] ? -1 : +1); sign -= 2) {
      TableOverride o;
      const int rc = perturb_tables(c->desc, c->slots(), c->tab, id, P.values(k, sign), o, c->err(), c->nwt.path == 1);
      if (rc != CH_OK) return rc;
      if (!o.src_par.empty() && transens_moves_breakpoints(c->desc.src, c->tab.src_par, o.src_par, c->tab.Ssrc, t0, t1)) {
        c->set_err("ch_tran_sens: slot " + std::to_string(id) + " (" + transens_src_field(c->desc.src[sa], c->desc.slot_b[id]) + " of source " + std::to_string(sa) +
                   ") moves a break point: the step sequence is not differentiable in that direction");
        return CH_ERR_UNSUPPORTED;
      }
    }
  }
  return CH_OK;
}

// the once-per-transient table sets and the buffers of the recursion
static int transens_build(ch_circuit* c, TranSens& T) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  const auto tb0 = hclock::now();
  const int S = T.S, n_par = T.n_par;
  hipStream_t st = c->ctx->stream;
  HIPCHK(c->ac.d_dumpG.alloc(T.nA)); HIPCHK(c->ac.d_dumpC.alloc(T.nA)); HIPCHK(c->ac.d_dumpA.alloc(T.nA)); HIPCHK(c->ac.d_dumpF0.alloc(T.nF)); HIPCHK(c->ac.d_dumpQ.alloc(T.nF));
  T.bmeta = c->ac_bmeta();
  if (!T.bmeta) return CH_ERR_DEVICE;
  ArenaScope own(nullptr);   // everything below lives as long as this call, not as long as the circuit
  T.plus.resize(n_par); T.minus.resize(n_par);
  for (int k = 0; k < n_par; ++k) for (int sign = +1; sign >= (T.plan.central[k] ? -1 : +1); sign -= 2) {
    std::unique_ptr<TranSensSet> set(new TranSensSet());
    set->a = c->nwt.base;
    const int rc = sens_perturb(c, T.plan.slot[k], T.plan.values(k, sign), set->o, set->a, &set->store);
    if (rc != CH_OK) return rc;
    set->lds_extra = set->o.lds_extra_doubles * sizeof(double);
    (sign > 0 ? T.plus : T.minus)[k] = std::move(set);
  }
  const size_t ring = transens_ring_doubles(n_par, S, T.nu);
  HIPCHK(T.d_S.alloc(ring)); HIPCHK(T.d_W.alloc(ring));
  HIPCHK(hipMemsetAsync(T.d_S.p, 0, ring * sizeof(double), st)); HIPCHK(hipMemsetAsync(T.d_W.p, 0, ring * sizeof(double), st));
  HIPCHK(T.d_Fp.alloc(T.nF * n_par)); HIPCHK(T.d_Fm.alloc(T.nF * n_par)); HIPCHK(T.d_Qp.alloc(T.nF * n_par)); HIPCHK(T.d_Qm.alloc(T.nF * n_par)); HIPCHK(T.d_Q0.alloc(T.nF));
  // (a forward slot never writes its minus columns and the kernel never reads them; cleared so that no launch reads fresh memory)
  HIPCHK(hipMemsetAsync(T.d_Fm.p, 0, T.nF * n_par * sizeof(double), st)); HIPCHK(hipMemsetAsync(T.d_Qm.p, 0, T.nF * n_par * sizeof(double), st));
  std::vector<int> zero(1, 0);
  HIPCHK(T.d_den.upload(T.plan.den, st)); HIPCHK(T.d_central.upload(T.plan.central, st)); HIPCHK(T.d_fail.upload(zero, st));
  T.kc = transens_chunk_columns(T.ds);
  if (T.ds > 96) {
    T.kc = std::min(T.kc, n_par);
    T.bchunk = sens_block_chunk(T.ds, T.kc, T.nblk);
    if (T.work.alloc((size_t)T.bchunk * sens_work_doubles(T.ds, T.kc)) != hipSuccess) { c->set_err("ch_tran_sens: out of device memory for the dense LU workspace"); return CH_ERR_DEVICE; }
  }
  T.rows.row_doubles = transens_row_doubles(T.n_obs, n_par, S);
  T.build_s = std::chrono::duration<double>(hclock::now() - tb0).count();
  return CH_OK;
}

// One point of the recursion: the evaluations at the state in ring slot x_slot (source time t, `mode` of source_value), then the solve.
// solve = true: s from (G + alpha[0] C) s = -[...] with k history slots, into ring slot `out`; false: s is already in `out`, only w is formed.
static int transens_point(ch_circuit* c, TranSens& T, int x_slot, int free_slot, double t, int mode, const double* alpha, int k, const int* hist_slot, int out, bool solve) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  const auto te0 = T.profile ? hclock::now() : hclock::time_point();
  const double ms0 = c->stats.device_ms;
  int rc = smallsignal_eval(c, c->nwt.base, c->own_sources(), 0, mode, c->ac.d_dumpF0.p, c->ac.d_dumpG.p, c->ac.d_dumpC.p, x_slot, free_slot, t, T.d_Q0.p);
  if (rc != CH_OK) return rc;
  ++T.n_eval;
  const SourceTables own = c->own_sources();
  for (int p = 0; p < T.n_par; ++p) for (int sign = +1; sign >= (T.plan.central[p] ? -1 : +1); sign -= 2) {
    const TranSensSet& set = *(sign > 0 ? T.plus : T.minus)[p];
    const SourceTables src{set.o.src_dc.empty() ? own.dc : &set.o.src_dc, set.o.src_par.empty() ? own.par : &set.o.src_par};
    rc = smallsignal_eval(c, set.a, src, set.lds_extra, mode, (sign > 0 ? T.d_Fp.p : T.d_Fm.p) + (size_t)p * T.nF, c->ac.d_dumpA.p, nullptr, x_slot, free_slot, t,
                          (sign > 0 ? T.d_Qp.p : T.d_Qm.p) + (size_t)p * T.nF);
    if (rc != CH_OK) return rc;
    ++T.n_eval;
  }
  if (T.profile) { T.eval_s += std::chrono::duration<double>(hclock::now() - te0).count(); T.eval_ms += (float)(c->stats.device_ms - ms0); }
  TranSensArgs a; std::memset(&a, 0, sizeof(a));
  a.bmeta = T.bmeta; a.G = c->ac.d_dumpG.p; a.C = c->ac.d_dumpC.p; a.F0 = c->ac.d_dumpF0.p; a.Q0 = T.d_Q0.p;
  a.Fp = T.d_Fp.p; a.Fm = T.d_Fm.p; a.Qp = T.d_Qp.p; a.Qm = T.d_Qm.p; a.den = T.d_den.p; a.central = T.d_central.p;
  a.Sr = T.d_S.p; a.Wr = T.d_W.p;
  for (int j = 0; j <= k && j < 6; ++j) a.alpha[j] = alpha[j];
  for (int j = 0; j < k && j < 5; ++j) a.hist_slot[j] = hist_slot[j];
  a.k = k; a.cand = out; a.solve = solve ? 1 : 0;
  a.f_stride = (long)T.nF; a.ds = T.ds; a.S = T.S; a.n_unk = T.nu; a.n_par = T.n_par; a.fail = T.d_fail.p;
  if (T.profile) HIPCHK(timed_begin(c));
  for (int k0 = 0; k0 < T.n_par; k0 += T.kc) {
    a.k0 = k0; a.kc = std::min(T.kc, T.n_par - k0);
    if (T.ds <= 96) {
      a.blk0 = 0; a.work = nullptr;
      hipLaunchKernelGGL(transens_step_kernel<64>, dim3(T.nblk), dim3(64), transens_lds_doubles(T.ds, a.kc) * sizeof(double), st, a);
      HIPCHK(hipGetLastError());
      ++T.n_solve_launches;
    } else for (int b0 = 0; b0 < T.nblk; b0 += T.bchunk) {
      a.blk0 = b0; a.work = T.work.p;
      hipLaunchKernelGGL(transens_step_kernel<256>, dim3(std::min(T.bchunk, T.nblk - b0)), dim3(256), 0, st, a);
      HIPCHK(hipGetLastError());
      ++T.n_solve_launches;
    }
    if (solve) ++T.n_factor_chunks;
  }
  if (T.profile) HIPCHK(timed_end(c, &T.solve_ms));   // profiling run: one synchronisation per point
  ++T.n_points; if (solve) ++T.n_solved;
  return CH_OK;
}

// ---- the hooks of the host stepper's loop (ch_engine_tran.hpp) ----
// one saved row of sensitivities beside saved row `row` of the states: the same weighted sum of ring slots
inline int ch_circuit::transens_save_row(long row, const int* slots, const double* w, int nw) {
  TranSens& T = *tsens;
  if (T.n_obs == 0) return CH_OK;
  double* dst = nullptr;
  HIPCHK(T.rows.row_ptr(row, &dst));
  SensObsArgs oa; oa.Sr = T.d_S.p; oa.nw = nw; oa.n_unk = T.nu; oa.S = T.S; oa.n_obs = T.n_obs; oa.n_par = T.n_par; oa.obs_unk = stru.d_obs_unk.p; oa.dst = dst;
  for (int j = 0; j < 8; ++j) { oa.slots[j] = j < nw ? slots[j] : 0; oa.w[j] = j < nw ? w[j] : 0.0; }
  const long n = (long)T.n_obs * T.n_par * T.S;
  hipLaunchKernelGGL(save_sens_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, oa);
  HIPCHK(hipGetLastError());
  return CH_OK;
}
// behind on_accept: the recursion's step at the accepted state, with the coefficients and history slots of the accepted attempt
inline int ch_circuit::transens_after_accept(const StepControl& sc, const ch_result& R) {
  TranSens& T = *tsens;
  const int newest = sc.order[0];
  const int rc = transens_point(this, T, newest, sc.order[NSLOT - 1], sc.source_time(), 1, sc.c.alpha, sc.c.k, sc.c.hist_slot, newest, true);
  if (rc != CH_OK) return rc;
  if (T.o->n_saveat == 0 && T.n_obs > 0) { const double one = 1.0; return transens_save_row((long)R.times.size(), &newest, &one, 1); }   // (otherwise save_row saves it)
  return CH_OK;
}

// the saved rows into [n_obs][n_par][n_times][S], then the rows the device does not own
static int transens_collect(ch_circuit* c, TranSens& T, ch_result& R) {
  const Analysis& A = c->desc.A;
  const int n_obs = T.n_obs, n_par = T.n_par, S = T.S;
  const size_t nt = R.times.size(), rd = T.rows.row_doubles;
  R.n_par = n_par;
  R.sens.assign((size_t)n_obs * n_par * nt * S, 0.0);
  if (hipStreamSynchronize(c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  std::vector<double> buf((size_t)RowStore::CH * rd);
  for (size_t ci = 0; ci < T.rows.chunks.size(); ++ci) {
    if (ci * RowStore::CH >= nt) break;
    const size_t nr = std::min<size_t>(RowStore::CH, nt - ci * RowStore::CH);
    if (rd == 0 || nr == 0) continue;
    if (hipMemcpy(buf.data(), T.rows.chunks[ci], nr * rd * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return CH_ERR_DEVICE;
    for (size_t r = 0; r < nr; ++r) for (int ob = 0; ob < n_obs; ++ob) for (int k = 0; k < n_par; ++k)
      std::copy(buf.begin() + r * rd + ((size_t)ob * n_par + k) * S, buf.begin() + r * rd + ((size_t)ob * n_par + k + 1) * S,
                R.sens.begin() + (((size_t)ob * n_par + k) * nt + ci * RowStore::CH + r) * S);
  }
  const int nsrc = (int)c->desc.src.size();
  const SourceTables own = c->own_sources();
  for (int ob = 0; ob < n_obs; ++ob) {
    double* row = &R.sens[(size_t)ob * n_par * nt * S];
    if (c->desc.obs_kind[ob] == 0 && A.node_unknown[c->desc.obs_index[ob]] < 0) {
      // a known node: the exact derivative of its value expression at every saved time
      const KnownDef& kd = A.known[A.node_known[c->desc.obs_index[ob]]];
      for (int k = 0; k < n_par; ++k) {
        const int sa = T.plan.src_of[k];
        const TableOverride* po = sa >= 0 ? &T.plus[k]->o : nullptr;
        for (size_t it = 0; it < nt; ++it) for (int s = 0; s < S; ++s) {
          double v = 0.0;
          if (sa >= 0) {
            const size_t at = (size_t)(c->tab.Ssrc > 1 ? s : 0) * nsrc + sa;
            const std::vector<double>& pp = po->src_par.empty() ? *own.par : po->src_par; const std::vector<double>& pd = po->src_dc.empty() ? *own.dc : po->src_dc;
            v = transens_known_deriv(kd, c->desc.src, sa, T.is_value[k] != 0, &pp[at * CH_SRC_NPAR], pd[at], &(*own.par)[at * CH_SRC_NPAR], (*own.dc)[at], T.plan.h[(size_t)k * S + s], R.times[it], 1);
          }
          row[((size_t)k * nt + it) * S + s] = v;
        }
      }
    } else if (c->desc.obs_kind[ob] == 1) {
      const int b = c->desc.dev[c->desc.obs_index[ob]].branch;
      // (the rule of finish_tran for the state rows; an observed voltage source keeps its branch, so no circuit built through the public
      //  interface gets here today)
      if (b < 0 || A.branch_unknown[b] < 0) std::fill(row, row + (size_t)n_par * nt * S, CH_NAN);
    }
  }
  return CH_OK;
}

static int transens_solve(ch_circuit* c, double t0, double t1, const ch_tran_opts& o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, ch_result& R) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  { const int vrc = c->check_tran_opts(t0, t1, o); if (vrc != CH_OK) return vrc; }
  ch_sens_opts sopt;
  { const int vrc = sens_check_args(c, "ch_tran_sens", n_par, slot_ids, nullptr, so, sopt, false); if (vrc != CH_OK) return vrc; }
  if (o.stepper == CH_STEPPER_DEVICE || c->torn.is_torn) { c->set_err("ch_tran_sens: transient sensitivities run on the host stepper only"); return CH_ERR_UNSUPPORTED; }
  const auto tstart = hclock::now();
  c->tran_reset(R);
  int rc = smallsignal_prepare(c, "transient sensitivities", "dense LU");
  if (rc != CH_OK) return rc;
  TranPlan p = resolve_tran_plan(t0, t1, o);
  TranSens T;
  T.n_par = n_par; T.S = c->tab.S; T.nblk = c->ac_ncomp() * T.S; T.ds = c->ac_ds(); T.nu = c->desc.A.n_unk; T.n_obs = R.n_obs; T.o = &o; T.profile = c->host_profile;
  T.nA = (size_t)T.nblk * T.ds * T.ds; T.nF = (size_t)T.nblk * T.ds;
  const auto tsets = hclock::now();
  rc = transens_steps(c, T, slot_ids, sopt, t0, t1);
  if (rc != CH_OK) return rc;
  rc = transens_build(c, T);
  if (rc != CH_OK) return rc;
  // ---- the state path of tran_solve on the host stepper: its own set-up, its own loop ----
  rc = c->tran_start(p, R, tstart, std::chrono::duration<double>(hclock::now() - tsets).count());
  if (rc != CH_OK) return rc;
  StepControl sc(p);
  RowStore rows; rows.row_doubles = (size_t)R.n_obs * c->tab.S;
  // ---- start: s_0 = the DC sensitivities at the transient's own operating point (0 with skip_dc: the ring is cleared), then
  //      w_0 = C s_0 + dq/dp at t0 in the transient's mode.  Slot 0 is the state at t0; the free slot takes the candidate rows. ----
  { const double a0[1] = {0.0}; const int free_slot = sc.order[NSLOT - 1];
    if (!o.skip_dc) { rc = transens_point(c, T, 0, free_slot, 0.0, o.dc.tran_mode ? 2 : 0, a0, 0, nullptr, sc.order[0], true); if (rc != CH_OK) return rc; }
    rc = transens_point(c, T, 0, free_slot, t0, 1, a0, 0, nullptr, sc.order[0], false); if (rc != CH_OK) return rc; }
  int status = CH_OK;
  { TranSensScope scope(c, &T);
    rc = c->host_stepper_run(p, R, sc, rows, status); }
  if (rc != CH_OK) return rc;
  c->host_stepper_collect(R, rows);
  status = c->finish_tran(R, sc.order[0], sc.t, status, tstart);
  rc = transens_collect(c, T, R);
  if (rc != CH_OK) { c->set_err("ch_tran_sens: reading the sensitivity rows back failed"); return rc; }
  int fail = 0;
  if (hipMemcpy(&fail, T.d_fail.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return CH_ERR_DEVICE;
  ch_stats& st = R.stats;
  st.n_kernel_launches += T.n_solve_launches; st.nf += (int64_t)T.n_eval * T.S; st.njacs += (int64_t)T.n_points * T.S;
  st.nfactors += (int64_t)T.nblk * T.n_factor_chunks; st.nsolve += (int64_t)T.nblk * T.n_par * T.n_solved;   // (the start's w_0 factors nothing)
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - tstart).count();
  if (T.profile)
    std::fprintf(stderr, "[transens] table sets %.3f ms (once), %ld points, %ld evaluation launches %.3f ms (host wall) / %.3f ms (HIP events, sampled launches), solve kernel %ld launches %.3f ms (HIP events), total %.3f ms\n",
                 T.build_s * 1e3, T.n_points, T.n_eval, T.eval_s * 1e3, (double)T.eval_ms, T.n_solve_launches, (double)T.solve_ms, st.wall_seconds * 1e3);
  if (status == CH_OK && fail) { c->set_err("transient sensitivities: singular matrix G + alpha0 C at an accepted step"); return CH_ERR_SINGULAR; }
  return status;
}

static int ch_tran_sens_impl(ch_circuit* c, double t0, double t1, const ch_tran_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, ch_result** out) {
  if (!c || !o || !out) return CH_ERR_INVALID;
  CallScope call(c);
  std::unique_ptr<ch_result> R(new ch_result());
  R->ctx = c->ctx;
  const int rc = transens_solve(c, t0, t1, *o, n_par, slot_ids, so, *R);
  R->status = rc;
  *out = R.release();
  return rc;
}
}  // extern "C++"
