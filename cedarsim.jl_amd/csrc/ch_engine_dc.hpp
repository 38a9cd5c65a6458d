// ch_engine_dc.hpp — the DC operating point: CedarDCOp + bootstrapped_nlsolve, restarted per block (src/dcop.jl:53-94).  Member
// functions of ch_circuit; included by ch_engine.hip behind the definition of ch_circuit.  The host arithmetic of the passes — the
// cached start vector, each restart's guess, the harvest of the statuses — is HIP-free in ch_dc_start.hpp; what is here moves the
// state between the ring slot and the host and launches the solves.
#pragma once

// The first pass without x0 starts every block from 1e-7*randn: the same numbers on every call with this (seed, S), drawn and
// uploaded once per circuit.  The restarts continue from the generators as that fill left them.
inline int ch_circuit::dc_start_vector(const ch_dc_opts& o) {
  const size_t slot_elems = (size_t)tab.S * desc.A.n_unk;
  if (dc_start.matches(o.seed, tab.S) && d_dc_start.p && d_dc_start.n >= slot_elems) return CH_OK;
  dc_start.valid = false;
  dc_start.fill(o.seed, tab.S, desc.A.n_mna, desc.A.unk_mna);
  const hipError_t ue = d_dc_start.upload(dc_start.xs, ctx->stream);
  if (ue != hipSuccess) { dc_start.valid = false; set_err(std::string("DC start vector: ") + hipGetErrorString(ue)); return CH_ERR_DEVICE; }
  return CH_OK;
}
// initial guess of pass r in ring slot `slot`, and the active mask the pass runs under
inline int ch_circuit::dc_guess(NewtonArgs& a, const ch_dc_opts& o, int slot, int r, bool homotopy, DcRestarts& P) {
  const size_t slot_elems = (size_t)tab.S * desc.A.n_unk;
  if (r == 0 && !o.x0) {
    // every block is active and every unknown takes its random start: one copy on the device, and no mask (null = all active)
    HIPCHK(hipMemcpyAsync(nwt.d_X.p + (size_t)slot * slot_elems, d_dc_start.p, slot_elems * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    a.active = nullptr;
    return CH_OK;
  }
  a.active = nwt.d_active.p;
  HIPCHK(hipMemcpy(P.xs.data(), nwt.d_X.p + (size_t)slot * slot_elems, P.xs.size() * sizeof(double), hipMemcpyDeviceToHost));
  P.guess(desc.A, r, homotopy, o.x0);
  HIPCHK(hipMemcpy(nwt.d_X.p + (size_t)slot * slot_elems, P.xs.data(), P.xs.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(nwt.d_active.p, P.active.data(), P.nblk, hipMemcpyHostToDevice));
  return CH_OK;
}
// one pass: a plain Newton solve, or (homotopy) gmin stepping: a shunt conductance on every node, relaxed decade by decade, then removed
inline int ch_circuit::dc_pass(NewtonArgs& a, const unsigned char* active, bool homotopy, Summary& sm) {
  if (homotopy)
    for (double g = 1e-2; g >= 1e-13 * 0.99; g *= 0.1) { a.gshunt = g; const int rc = run_newton(a, active, sm); if (rc != CH_OK) return rc; }
  a.gshunt = 0.0;
  return run_newton(a, active, sm);
}
// the blocks' statuses of the pass -> P, which retires the converged ones
inline int ch_circuit::dc_harvest(DcRestarts& P) {
  if (nwt.path == 2) { for (int b = 0; b < P.nblk; ++b) P.status[b] = sp.newton.status_v[b % tab.S]; }
  else if (nwt.host_reduce) { for (int b = 0; b < P.nblk; ++b) P.status[b] = nwt.h_out[b].status; }
  else {
    std::vector<BlockOut> bo(P.nblk);
    HIPCHK(hipMemcpy(bo.data(), nwt.d_out.p, P.nblk * sizeof(BlockOut), hipMemcpyDeviceToHost));
    for (int b = 0; b < P.nblk; ++b) P.status[b] = bo[b].status;
  }
  P.harvest();
  return CH_OK;
}

// Leaves the solution in ring slot `slot`.
inline int ch_circuit::dc_solve(const ch_dc_opts& o, int slot, std::vector<int>* status_out, ch_stats* stt) {
  NewtonArgs a = nwt.base;
  a.mode = MODE_DC; a.maxit = std::max(1, o.maxiters); a.dc_abstol = o.abstol; a.dv_max = o.dv_max; a.gshunt = 0.0;
  a.abstol = 1e-6; a.reltol = 1e-3; a.newton_tol = 0.1;
  a.hist_slot[0] = slot; a.cand_slot = slot; a.active = nwt.d_active.p;
  int rc = set_sources(a, 0.0, o.tran_mode ? 2 : 0);
  if (rc != CH_OK) return rc;
  LapTimer lt(host_profile);   // ("DC wait" is all of run_newton)
  if (!o.x0) { rc = dc_start_vector(o); if (rc != CH_OK) return rc; }
  DcRestarts P(desc.A, tab.S, o.x0 ? dc_start_rngs(o.seed, tab.S) : dc_start.after);
  lt.lap(laps.start_vector);
  const int nrest = std::max(1, o.n_restarts);
  for (int r = 0; r < nrest + 1 && P.n_active > 0; ++r) {
    const bool homotopy = (r == nrest);
    rc = dc_guess(a, o, slot, r, homotopy, P);
    if (rc != CH_OK) return rc;
    lt.lap(laps.dc_copies);
    Summary sm;
    rc = dc_pass(a, P.active.data(), homotopy, sm);
    if (rc != CH_OK) return rc;
    lt.lap(laps.dc_wait);
    if (stt) add_newton_iters(*stt, sm.sum_iters, sm.sum_block_iters);
    rc = dc_harvest(P);
    if (rc != CH_OK) return rc;
    if (P.n_active > 0 && stt) { stt->nrestarts++; stt->nnonlinconvfail++; }
    lt.lap(laps.dc_copies);
  }
  if (status_out) P.sample_status(*status_out);
  if (P.n_active > 0) { set_err("DC operating point analysis failed for " + std::to_string(P.n_active) + " block(s)"); return CH_ERR_MAXITERS; }
  return CH_OK;
}
