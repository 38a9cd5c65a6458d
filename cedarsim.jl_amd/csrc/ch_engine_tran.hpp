// ch_engine_tran.hpp — the transient driver: the checks on a request, its named steps (initial state, charges at t0, the device
// stepper where the circuit qualifies, else the host stepper's attempt loop and its rows) and the end both steppers share.  Member
// functions of ch_circuit; included by ch_engine.hip behind the definition of ch_circuit.  The resolved request (TranPlan), the
// break points and the step controller are HIP-free in ch_stepper_host.hpp; the device stepper's launch is in ch_engine_persist.hpp.
#pragma once

// what no solver below should have to defend against: non-finite spans and tolerances, an output grid that is not a grid
inline int ch_circuit::check_tran_opts(double t0, double t1, const ch_tran_opts& o) {
  if (!std::isfinite(t0) || !std::isfinite(t1) || !(t1 > t0)) { set_err("tspan must be finite and increasing"); return CH_ERR_INVALID; }
  if (!(o.abstol >= 0) || !(o.reltol >= 0) || !std::isfinite(o.abstol) || !std::isfinite(o.reltol) || o.abstol + o.reltol == 0) { set_err("abstol and reltol must be finite, non-negative and not both zero"); return CH_ERR_INVALID; }
  if (!(o.dtmin >= 0) || !(o.dtmax >= 0) || !(o.dt0 >= 0) || !std::isfinite(o.dtmin) || !std::isfinite(o.dtmax) || !std::isfinite(o.dt0)) { set_err("dtmin, dtmax and dt0 must be finite and non-negative (0 = automatic)"); return CH_ERR_INVALID; }
  if (o.n_saveat < 0 || (o.n_saveat > 0 && !o.saveat)) { set_err("saveat: n_saveat points announced, none given"); return CH_ERR_INVALID; }
  for (int i = 0; i < o.n_saveat; ++i)
    if (!std::isfinite(o.saveat[i]) || (i > 0 && o.saveat[i] < o.saveat[i - 1])) { set_err("saveat must be finite and non-decreasing"); return CH_ERR_INVALID; }
  if (o.stepper < CH_STEPPER_AUTO || o.stepper > CH_STEPPER_DEVICE) { set_err("stepper must be CH_STEPPER_AUTO, _HOST or _DEVICE"); return CH_ERR_INVALID; }
  if (o.step_control != CH_STEPS_AUTO && o.step_control != CH_STEPS_SHARED) { set_err("step_control must be CH_STEPS_AUTO or CH_STEPS_SHARED"); return CH_ERR_INVALID; }
  return CH_OK;
}

// ---- initialisation: the state at t0 goes to ring slot 0, the newest slot of a fresh StepControl ----
inline int ch_circuit::tran_initial_state(const ch_tran_opts& o, ch_result& R) {
  if (!o.skip_dc) return dc_solve(o.dc, 0, nullptr, &R.stats);
  if (o.dc.x0) return upload_from_mna(0, o.dc.x0);
  if (!torn.keep_slot0) HIPCHK(hipMemsetAsync(nwt.d_X.p, 0, (size_t)tab.S * desc.A.n_unk * sizeof(double), ctx->stream));
  return CH_OK;
}
// charges at t0 in the problem's own mode
inline int ch_circuit::tran_charges_at_t0(double t0, const ch_tran_opts& o, ch_result& R) {
  LapTimer lt(host_profile);
  NewtonArgs a = nwt.base; a.mode = MODE_EVAL; a.maxit = 1; a.hist_slot[0] = 0; a.cand_slot = 0; a.abstol = o.abstol; a.reltol = o.reltol;
  int rc = set_sources(a, t0, 1); if (rc != CH_OK) return rc;
  Summary sm; rc = run_newton(a, nullptr, sm); if (rc != CH_OK) return rc;
  R.stats.nf += tab.S;
  lt.lap(laps.charges);
  return CH_OK;
}

// ---- device-resident step controller (ch_persist.hpp) where the circuit qualifies ----
// done = true: the transient has been dealt with (result or error in the return value); false: the host stepper takes it
inline int ch_circuit::try_device_stepper(const TranPlan& p, ch_result& R, hclock::time_point tstart, bool& done) {
  done = true;
  const ch_tran_opts& o = *p.o;
  const int want = resolve_stepper(o.stepper, env_get(Env::STEPPER));
  if (want != CH_STEPPER_HOST) {
    std::string why;
    if (persist_eligible(why, persist_own_steps(o))) {
      ps.aborted = false;
      const PersistStep s = tran_persistent(p, R, tstart);
      if (s.launched() && ps.aborted && want != CH_STEPPER_DEVICE) {
        // A grid-wide wait ran into its bound: the cooperative launch shared the GPU with another process's kernel and
        // its workgroups were not all resident.  The solve is repeated on the host stepper (whose launches need no
        // co-residency); the torn form hands back to the sparse path of its parent.
        const std::string msg = err();
        ctx->err.clear();
        if (torn.is_torn) { set_err(msg); return CH_ERR_UNSUPPORTED; }
        ch_tran_opts o3 = o; o3.stepper = CH_STEPPER_HOST;
        return tran_solve(p.t0, p.t1, o3, R);
      }
      if (s.launched()) return s.rc;
      why = err();   // declined, or an error in front of the first launch: the host stepper takes the transient
    }
    if (want == CH_STEPPER_DEVICE || torn.is_torn) { set_err("device-resident stepper not available for this circuit: " + why); return CH_ERR_UNSUPPORTED; }
    if (env_on(Env::DEBUG_STEPPER)) std::fprintf(stderr, "[stepper] host stepper because: %s\n", why.c_str());
  }
  if (torn.is_torn) { set_err("the torn form of a circuit runs on the device-resident stepper only"); return CH_ERR_UNSUPPORTED; }
  done = false;
  return CH_OK;
}

// ---- host step controller (StepControl, ch_stepper_host.hpp): one Newton launch per attempt ----
// saved observables of the host stepper live on the device until the end: rows [row][obs][sample] in chunks of CH rows
struct RowStore {
  static constexpr int CH = 512;
  std::vector<double*> chunks; size_t row_doubles = 1;
  ~RowStore() { for (double* p : chunks) (void)hipFree(p); }   // freed on every exit, exceptions included
  // device address of saved-row `row`, growing the buffer by chunks
  hipError_t row_ptr(long row, double** out) {
    while ((size_t)(row / CH) >= chunks.size()) { double* p = nullptr; const hipError_t e = hipMalloc((void**)&p, std::max<size_t>(1, (size_t)CH * row_doubles) * sizeof(double)); if (e != hipSuccess) return e; chunks.push_back(p); }
    *out = chunks[row / CH] + (size_t)(row % CH) * row_doubles;
    return hipSuccess;
  }
};
// one saved row at time ts: the weighted sum of ring slots `slots` (save_obs_kernel)
inline int ch_circuit::save_row(ch_result& R, RowStore& rows, double ts, const int* slots, const double* w, int nw) {
  double* dst = nullptr;
  HIPCHK(rows.row_ptr((long)R.times.size(), &dst));
  if (tsens) { const int rcs = transens_save_row((long)R.times.size(), slots, w, nw); if (rcs != CH_OK) return rcs; }   // ch_tran_sens: the same row of the S ring
  const int n_obs = R.n_obs;
  if (n_obs > 0) {
    ObsArgs oa; oa.X = nwt.d_X.p; oa.slot_stride = (long)tab.S * desc.A.n_unk; oa.nw = nw; oa.n_unk = desc.A.n_unk; oa.S = tab.S; oa.n_obs = n_obs; oa.obs_unk = stru.d_obs_unk.p;
    for (int j = 0; j < nw; ++j) { oa.slots[j] = slots[j]; oa.w[j] = w[j]; }
    oa.dst = dst;
    const int n = n_obs * tab.S;
    hipLaunchKernelGGL(save_obs_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, oa);
  }
  R.times.push_back(ts); R.pts.push_back(0);
  return CH_OK;
}
// the attempt loop -> status: how the transient ended (CH_OK: t1 reached); returns an error only where the first rows cannot be saved
inline int ch_circuit::host_stepper_run(const TranPlan& p, ch_result& R, StepControl& sc, RowStore& rows, int& status) {
  const ch_tran_opts& o = *p.o;
  const int n_obs = R.n_obs;
  int rc = CH_OK, isave = 0;
  status = CH_OK;
  { const double one = 1.0; const int s0 = sc.order[0];
    if (o.n_saveat == 0) { rc = save_row(R, rows, p.t0, &s0, &one, 1); if (rc) return rc; }
    else while (isave < o.n_saveat && o.saveat[isave] <= p.t0) { rc = save_row(R, rows, o.saveat[isave], &s0, &one, 1); if (rc) return rc; ++isave; } }
  NewtonArgs a = nwt.base;
  a.mode = MODE_TRAN; a.maxit = p.nmaxit; a.abstol = o.abstol; a.reltol = o.reltol; a.newton_tol = 0.1;
  for (int step = 0; step < p.max_steps && sc.t < p.t1;) {
    status = sc.plan();
    if (status != CH_OK) break;
    const StepCoeffs& c = sc.c;
    a.k = c.k; a.npred = c.npred; a.nkm1 = c.nkm1; a.nkp1 = c.nkp1; a.ck = c.ck; a.ckm1 = c.ckm1; a.ckp1 = c.ckp1; a.cand_slot = c.cand_slot;
    std::memcpy(a.alpha, c.alpha, sizeof(a.alpha)); std::memcpy(a.wpred, c.wpred, sizeof(a.wpred)); std::memcpy(a.wkm1, c.wkm1, sizeof(a.wkm1)); std::memcpy(a.wkp1, c.wkp1, sizeof(a.wkp1));
    std::memcpy(a.hist_slot, c.hist_slot, sizeof(a.hist_slot));
    rc = set_sources(a, sc.source_time(), 1); if (rc != CH_OK) { status = rc; break; }
    a.reset_rate = sc.reset_rate ? 1 : 0;
    a.obs_row = nullptr;
    if (o.n_saveat == 0 && n_obs > 0 && rows.row_ptr((long)R.times.size(), &a.obs_row) != hipSuccess) { set_err("host stepper: out of device memory for the saved rows"); status = CH_ERR_DEVICE; break; }  // candidate row, kept on accept
    Summary sm;
    rc = run_newton(a, nullptr, sm); if (rc != CH_OK) { status = rc; break; }
    R.stats.n_step_attempts++;
    add_newton_iters(R.stats, sm.sum_iters, sm.sum_block_iters);
    if (sm.n_fail > 0) { R.stats.nnonlinconvfail++; sc.on_convergence_failure(); continue; }
    const double errk = sc.lte ? sm.errk : 0.0;
    if (errk > 1.0) { R.stats.nreject++; sc.on_error_test_failure(errk); continue; }
    R.stats.naccept++; ++step;
    sc.on_accept();
    if (tsens) { rc = transens_after_accept(sc, R); if (rc != CH_OK) { status = rc; break; } }   // ch_tran_sens: the recursion's step, in front of the rows
    if (o.n_saveat > 0) {
      while (isave < o.n_saveat && o.saveat[isave] <= sc.tn * (1 + 1e-15)) {
        double ww[9]; const int m = sc.dense_weights(o.saveat[isave], ww);
        rc = save_row(R, rows, o.saveat[isave], sc.order, ww + 1, m); if (rc) break;
        ++isave;
      }
    } else if (n_obs > 0) { R.times.push_back(sc.tn); R.pts.push_back(sc.dense_points()); }  // the kernel's epilogue already wrote this row
    else { const double one = 1.0; rc = save_row(R, rows, sc.tn, sc.order, &one, 1); if (rc == CH_OK) R.pts.back() = sc.dense_points(); }
    if (rc != CH_OK) { status = rc; break; }
    sc.select_next(errk, sm.errkm1, sm.errkp1);
  }
  if (status == CH_OK && sc.t < p.t1) status = CH_ERR_MAXSTEPS;
  return CH_OK;
}
// the saved rows, chunk by chunk, into the result's layout
inline void ch_circuit::host_stepper_collect(ch_result& R, const RowStore& rows) {
  (void)hipStreamSynchronize(ctx->stream);
  const int n_obs = R.n_obs;
  const size_t nt = R.times.size();
  R.values.assign((size_t)n_obs * nt * tab.S, 0.0);
  std::vector<double> buf((size_t)RowStore::CH * n_obs * tab.S);
  for (size_t cidx = 0; cidx < rows.chunks.size(); ++cidx) {
    const size_t nr = std::min<size_t>(RowStore::CH, nt - cidx * RowStore::CH);
    if (n_obs == 0 || nr == 0) continue;
    (void)hipMemcpy(buf.data(), rows.chunks[cidx], nr * n_obs * tab.S * sizeof(double), hipMemcpyDeviceToHost);
    rows_to_obs_major(buf.data(), nr, cidx * RowStore::CH, nt, n_obs, tab.S, R.values.data());
  }
}

// a fresh result and fresh launch statistics: what every transient (ch_tran, ch_tran_sens) starts from
inline void ch_circuit::tran_reset(ch_result& R) {
  R.times.clear(); R.pts.clear(); R.values.clear(); R.final_state.clear(); R.sens.clear(); R.n_par = 0;   // (a launch that gave up may have left the rows of its first attempt)
  std::memset(&R.stats, 0, sizeof(R.stats));
  R.S = tab.S; R.n_obs = (int)desc.obs_kind.size();
  stats.reset(); laps = HostLaps();
}
// Everything in front of a stepper's first attempt, shared by ch_tran and ch_tran_sens: the state at t0 in ring slot 0, its charges,
// the plan's break points, identity pivot orders.  other_seconds: host time since tstart that was not initialisation (dc_seconds
// leaves it out)
inline int ch_circuit::tran_start(TranPlan& p, ch_result& R, hclock::time_point tstart, double other_seconds) {
  const ch_tran_opts& o = *p.o;
  int rc = tran_initial_state(o, R);
  if (rc != CH_OK) return rc;
  R.stats.dc_seconds = std::chrono::duration<double>(hclock::now() - tstart).count() - other_seconds;
  rc = tran_charges_at_t0(p.t0, o, R);
  if (rc != CH_OK) return rc;
  stats.end_of_dc(R.stats.n_block_iters);   // everything so far was initialisation
  collect_breakpoints(desc.src, tab.src_par, tab.Ssrc, p.t0, p.t1, p.bps, p.bpc);
  // every transient starts its blocks' LU pivot orders from the identity (see ch_persist.hpp: identical blocks stay identical);
  // once, in front of either stepper: a resumed launch reads what the launch before it left there
  if (nwt.d_perm.p) HIPCHK(hipMemsetAsync(nwt.d_perm.p, 0, (size_t)desc.A.n_comp * tab.S * 16, ctx->stream));
  return CH_OK;
}

inline int ch_circuit::tran_solve(double t0, double t1, const ch_tran_opts& o, ch_result& R) {
  { const int vrc = check_tran_opts(t0, t1, o); if (vrc != CH_OK) return vrc; }
  if (torn.c && !torn.is_torn && tab.S == 1 && !env_on(Env::NO_TEAR) && resolve_stepper(o.stepper, env_get(Env::STEPPER), false) != CH_STEPPER_HOST) {
    bool used = false;
    const int rc = tran_torn(t0, t1, o, R, used);
    if (used || rc != CH_OK) return rc;
  }
  auto tstart = hclock::now();
  tran_reset(R);
  int rc = finalize_params();
  if (rc != CH_OK) return rc;
  TranPlan p = resolve_tran_plan(t0, t1, o);
  rc = tran_start(p, R, tstart);
  if (rc != CH_OK) return rc;
  { bool done = false;
    rc = try_device_stepper(p, R, tstart, done);
    if (done) return rc; }
  StepControl sc(p);
  RowStore rows; rows.row_doubles = (size_t)R.n_obs * tab.S;
  int status = CH_OK;
  rc = host_stepper_run(p, R, sc, rows, status);
  if (rc != CH_OK) return rc;
  host_stepper_collect(R, rows);
  return finish_tran(R, sc.order[0], sc.t, status, tstart);
}

// shared end of both step controllers: derived observables, final state, statistics
// xs_final: the newest slot's unknowns [S][n_unk] where the caller has read them back already, or null
inline int ch_circuit::finish_tran(ch_result& R, int newest_slot, double t, int status, hclock::time_point tstart, const double* xs_final) {
  LapTimer lt(host_profile);
  const int n_obs = R.n_obs;
  const size_t nt = R.times.size();
  {
    // several observables fed by one unknown (merged nodes): the kernel writes the primary one only
    for (int ob = 0; ob < n_obs; ++ob) if (stru.obs_primary[ob] != ob)
      std::memcpy(&R.values[(size_t)ob * nt * tab.S], &R.values[(size_t)stru.obs_primary[ob] * nt * tab.S], nt * tab.S * sizeof(double));
    // observables that are known nodes / ground are evaluated on the host
    const int nk = (int)desc.A.known.size();
    std::vector<double> sv, kv;
    for (int ob = 0; ob < n_obs; ++ob) {
      if (desc.obs_kind[ob] == 0 && desc.A.node_unknown[desc.obs_index[ob]] < 0) {
        const int kn = desc.A.node_known[desc.obs_index[ob]];
        for (size_t it = 0; it < nt; ++it) { eval_sources(R.times[it], 1, sv, kv); for (int s = 0; s < tab.S; ++s) R.values[((size_t)ob * nt + it) * tab.S + s] = kv[(size_t)(tab.Ssrc > 1 ? s : 0) * nk + kn]; }
      } else if (desc.obs_kind[ob] == 1) {
        const int b = desc.dev[desc.obs_index[ob]].branch;
        if (b < 0 || desc.A.branch_unknown[b] < 0) for (size_t it = 0; it < nt; ++it) for (int s = 0; s < tab.S; ++s) R.values[((size_t)ob * nt + it) * tab.S + s] = CH_NAN;
      }
    }
  }
  R.final_state.assign((size_t)tab.S * desc.A.n_mna, 0.0);
  if (xs_final) unknowns_to_mna(xs_final, t, 1, R.final_state.data()); else download_mna(newest_slot, t, 1, R.final_state.data());
#ifdef CH_STAMPS
  { unsigned long long hs[8]; (void)hipMemcpy(hs, stru.d_stamps.p, sizeof(hs), hipMemcpyDeviceToHost);
    std::fprintf(stderr, "[stamps] cycles summed over blocks: prologue %llu eval %llu gather %llu solve %llu epilogue %llu arrival %llu pre-LU %llu LU %llu ; launches %ld blocks %d\n", hs[0], hs[1], hs[2], hs[3], hs[4], hs[5], hs[6], hs[7], stats.n_launch, desc.A.n_comp * tab.S); }
#endif
  R.status = status;
  R.stats.wall_seconds = std::chrono::duration<double>(hclock::now() - tstart).count();
  if (host_profile) { lt.lap(laps.collect);
    std::fprintf(stderr, "[host profile] wall %.3f ms; in run_newton: launch %.3f ms, wait %.3f ms, events+reduce %.3f ms; launches %ld\n", 1e3 * R.stats.wall_seconds, 1e3 * stats.prof_launch, 1e3 * stats.prof_wait, 1e3 * stats.prof_reduce, stats.n_launch); stats.prof_launch = stats.prof_wait = stats.prof_reduce = 0;
    std::fprintf(stderr, "[host laps] ms: start vector %.3f, DC copies %.3f, DC wait %.3f, charges launch %.3f, constants %.3f, launch->sync %.3f, read-back %.3f, collect %.3f\n", 1e3 * laps.start_vector, 1e3 * laps.dc_copies,
                 1e3 * laps.dc_wait, 1e3 * laps.charges, 1e3 * laps.consts, 1e3 * laps.launch_sync, 1e3 * laps.readback, 1e3 * laps.collect); }
  stats.fill(R.stats);
  R.stats.n_kernel_launches = stats.n_launch + stats.persist_launches;
  R.stats.n_step_attempts += stats.persist_attempts; R.stats.barrier_seconds = stats.persist_barrier_s;
  R.stats.stepper = stats.persist_launches > 0 ? CH_STEPPER_DEVICE : CH_STEPPER_HOST;
  R.stats.stepper_mode = stats.persist_launches > 0 ? ps.mode : 0;
  R.stats.step_block_iters = R.stats.n_block_iters - stats.dc_block_iters;
  if (status != CH_OK && err().empty()) set_err(status == CH_ERR_DTMIN ? "step size underflow (DtLessThanMin)" : "transient did not reach t1");
  return status;
}
