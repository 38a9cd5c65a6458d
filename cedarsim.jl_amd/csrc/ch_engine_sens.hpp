// ch_engine_sens.hpp — DC parameter sensitivities by the direct method (ch_dc_sens): F(x, p) = 0  =>  G · dx/dp_k = -dF/dp_k at x*.
// The operating point and G come from the linearisation the small-signal analyses use (slot 0 of the state ring, smallsignal_linearise
// in ch_engine_ac.hpp); dF/dp_k is a difference of two more MODE_EVAL launches (smallsignal_eval, ibid.) in which ONLY the table the slot reaches is replaced by a perturbed copy
// (NewtonArgs carries the tables as pointers; the copies come from perturb_tables, ch_param_tables.hpp, out of the host tables
// finalize_params kept): no finalize_params rebuild, no second Newton solve, no read-back, and the circuit's own tables are never
// written.  The step plan (SensPlan) and the MNA expansion are HIP-free (ch_sens_host.hpp); the solves run in sens_block_kernel.
// AC parameter sensitivities (ch_ac_sens, further down) share that front half — operating point, perturbed evaluations, real solves —
// and add the differences of the G, C dumps, acsens_rhs_kernel and acsens_solve_kernel; their HIP-free half is ch_acsens_host.hpp.
// What ch_noise_sens (ch_engine_noisesens.hpp) shares with ch_ac_sens is here as well: the buffers and the two terms of dY/dp
// (acsens_alloc_differences, acsens_explicit_term, acsens_state_term), the launcher of the frequency-chunked complex solves
// (launch_freq_chunks) and the rule every driver's return code follows (sens_outcome).  Included by ch_engine.hip behind ch_engine_ac.hpp.
#pragma once

extern "C++" {   // (included inside the extern "C" block of ch_engine.hip; templates need C++ linkage)

// The tables of one perturbed evaluation: slot `id` takes val[s] in sample s, everything else stays.  perturb_tables
// (ch_param_tables.hpp) makes the copies from the circuit's retained host tables; they go into the scratch buffers c->sens and `a`
// points at them.  The source tables stay on the host, in `o`.
// store: the device copies go there instead (the transient sensitivities keep one set per (parameter, sign) for a whole transient).
static int sens_perturb(ch_circuit* c, int id, const std::vector<double>& val, TableOverride& o, NewtonArgs& a, Sensitivity* store = nullptr) {
  hipStream_t st = c->ctx->stream; Sensitivity& d = store ? *store : c->sens;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  const int rc = perturb_tables(c->desc, c->slots(), c->tab, id, val, o, c->err(), c->nwt.path == 1);
  if (rc != CH_OK) return rc;
  if (!o.dpar.empty()) { HIPCHK(d.d_dpar.upload(o.dpar, st)); a.dpar = d.d_dpar.p; }
  if (!o.dmult.empty()) { HIPCHK(d.d_dmult.upload(o.dmult, st)); a.dmult = d.d_dmult.p; }
  if (!o.gmin.empty()) { HIPCHK(d.d_gmin.upload(o.gmin, st)); a.gmin_s = d.d_gmin.p; }
  if (!o.temp.empty()) { HIPCHK(d.d_temp.upload(o.temp, st)); a.temp_s = d.d_temp.p; }
  if (!o.vapar.empty()) { HIPCHK(d.d_vapar.upload(o.vapar, st)); a.vapar = d.d_vapar.p; }
  if (!o.mosp.empty()) { HIPCHK(d.d_mosp.upload(o.mosp, st)); a.mosp = d.d_mosp.p; }
  if (!o.dcls.empty()) { HIPCHK(d.d_dcls.upload(o.dcls, st)); a.dcls = d.d_dcls.p; }
  if (!o.bmeta.empty()) {
    HIPCHK(d.d_bmeta.upload(o.bmeta, st)); HIPCHK(d.d_dcls_local.upload(o.dcls_local, st)); HIPCHK(d.d_mc_list.upload(o.mc_list, st));
    a.bmeta = d.d_bmeta.p; a.dcls_local = d.d_dcls_local.p; a.mc_list = d.d_mc_list.p;
  }
  a.mos_cols = o.mos_cols; a.n_mos_cls = o.n_mos_cls; a.max_mc = o.max_mc;
  if (o.va_setup && c->stru.n_va_inst > 0) {
    const int rcv = c->launch_va_setup(a.vapar, a.temp_s, d.d_vacache);
    if (rcv != CH_OK) return rcv;
    a.vacache = d.d_vacache.p;
  }
  return CH_OK;
}

// G · X = B for every (block, sample) and the columns k0 .. k0+kc of the right-hand sides, in chunks that fit; *ms_out (zero at the
// call) takes the event time
static int launch_sens(ch_circuit* c, SensArgs& a, int nblk, int n_par, size_t nF, float* ms_out, int* n_chunks, int* n_launches) {
  *n_chunks = 0; *n_launches = 0;
  const int ds = a.ds;
  hipStream_t st = c->ctx->stream;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  HIPCHK(timed_begin(c));
  auto chunk_args = [&](int k0, int kmax, int b0, double* work) {   // columns k0 .. k0 + kmax of the blocks from b0 on
    SensArgs b = a;
    b.k0 = k0; b.kc = std::min(kmax, n_par - k0); b.blk0 = b0; b.work = work;
    b.Fp = a.Fp + (size_t)k0 * nF; b.Fm = a.Fm + (size_t)k0 * nF; b.den = a.den + (size_t)k0 * a.S;
    return b;
  };
  if (ds <= 96) {
    const int kmax = sens_lds_chunk_columns(ds);
    for (int k0 = 0; k0 < n_par; k0 += kmax) {
      const SensArgs b = chunk_args(k0, kmax, 0, nullptr);
      const size_t lds = (size_t)ds * sens_lda(ds, b.kc) * sizeof(double);
      hipLaunchKernelGGL(sens_block_kernel<64>, dim3(nblk), dim3(64), lds, st, b);
      HIPCHK(hipGetLastError());
      *n_launches += 1; *n_chunks += 1;
    }
  } else {
    const int kmax = sens_work_columns(n_par), bchunk = sens_block_chunk(ds, kmax, nblk);
    auto failed = [&]() { c->set_err("ch_dc_sens: the dense solve failed on the device"); return (int)CH_ERR_DEVICE; };
    ScopedWorkspace work;
    if (work.alloc((size_t)bchunk * sens_work_doubles(ds, kmax)) != hipSuccess) { c->set_err("ch_dc_sens: out of device memory for the dense LU workspace"); return CH_ERR_DEVICE; }
    for (int k0 = 0; k0 < n_par; k0 += kmax) for (int b0 = 0; b0 < nblk; b0 += bchunk) {
      hipLaunchKernelGGL(sens_block_kernel<256>, dim3(std::min(bchunk, nblk - b0)), dim3(256), 0, st, chunk_args(k0, kmax, b0, work.p));
      if (hipGetLastError() != hipSuccess) return failed();
      *n_launches += 1; if (b0 == 0) *n_chunks += 1;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return failed();
  }
  HIPCHK(timed_end(c, ms_out));
  return CH_OK;
}

// ---- the front half ch_dc_sens and ch_ac_sens share: operating point, perturbed evaluations (den, dsrc), real solves ----
struct SensRun {
  ch_sens_opts opt; ch_stats st; hclock::time_point t0, t_eval0, t_eval1, t_state0, t_state1;
  std::vector<int> status, skip; int rc_dc = CH_OK; std::string dc_err;
  int mode = 0, S = 0, nblk = 0, ds = 0, n_eval = 0, n_state = 0; size_t nA = 0, nF = 0;   // n_state: parameters that took the state pass
  SensPlan plan;                     // slot, kind of difference and source per parameter; step and divisor per (parameter, sample)
  std::vector<double> dsrc;          // [n_par][S]: d(source value)/dp for the rows of known nodes
  std::vector<double> xs;            // [S][n_par][n_unk]: dx*/dp in unknown order (also on the device, c->sens.d_x)
  float solve_ms = 0.0f; int n_chunks = 0, n_solve_launches = 0, fail = 0;
};

// has_out = false: the entry point has no output array of its own (ch_tran_sens returns a result handle), sens_out is not looked at
static int sens_check_args(ch_circuit* c, const char* who, int32_t n_par, const int32_t* slot_ids, const void* sens_out, const ch_sens_opts* so, ch_sens_opts& sopt,
                           bool has_out = true) {
  const std::string w(who);
  if (n_par < 1 || !slot_ids || (has_out && !sens_out)) { c->set_err(w + ": at least one parameter slot" + (has_out ? " and an output array" : "")); return CH_ERR_INVALID; }
  for (int k = 0; k < n_par; ++k) if (slot_ids[k] < 0 || slot_ids[k] >= (int)c->desc.slot_kind.size()) { c->set_err(w + ": slot id out of range"); return CH_ERR_INVALID; }
  ch_sens_opts_default(&sopt);
  if (so) sopt = *so;
  if (!(sopt.rel_step > 0.0) || !std::isfinite(sopt.rel_step)) { c->set_err(w + ": rel_step must be positive and finite"); return CH_ERR_INVALID; }
  return CH_OK;
}

// the step plan of a call (ch_sens_host.hpp) from the circuit's slot tables and current slot values
static SensPlan sens_plan_of(ch_circuit* c, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts& opt) {
  return sens_plan(c->desc.slot_kind, c->desc.slot_a, c->desc.dev, c->desc.A, (int)c->desc.src.size(), n_par, slot_ids, c->tab.S,
                   [&](int id, int s) { return c->slot_value(id, s); }, opt);
}

// operating point (slot 0; a sample that fails keeps its status, the others are served), then G, C and F there
static int sens_operating_point(ch_circuit* c, const ch_dc_opts* o, const char* what, int n_par, double* x_out, int32_t* status_out, SensRun& R) {
  R.t0 = hclock::now();
  std::memset(&R.st, 0, sizeof(R.st));
  c->stats.reset();
  int rc = smallsignal_prepare(c, what, "dense LU");
  if (rc != CH_OK) return rc;
  R.rc_dc = c->dc_solve(*o, 0, &R.status, &R.st);
  if (R.rc_dc != CH_OK && R.status.empty()) return R.rc_dc;
  R.dc_err = c->err();
  R.skip.assign(R.status.size(), 0);
  for (size_t s = 0; s < R.status.size(); ++s) R.skip[s] = R.status[s] != CH_OK;
  R.mode = o->tran_mode ? 2 : 0;
  if (x_out) { rc = c->download_mna(0, 0.0, R.mode, x_out); if (rc != CH_OK) return rc; }
  const Analysis& A = c->desc.A;
  R.S = c->tab.S; R.nblk = c->ac_ncomp() * R.S; R.ds = c->ac_ds();
  if (status_out) for (int s = 0; s < R.S; ++s) status_out[s] = R.status[s];
  R.st.dc_seconds = std::chrono::duration<double>(hclock::now() - R.t0).count();
  c->stats.end_of_dc(R.st.n_block_iters);
  R.nA = (size_t)R.nblk * R.ds * R.ds; R.nF = (size_t)R.nblk * R.ds;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  HIPCHK(c->sens.d_Fp.alloc(R.nF * n_par)); HIPCHK(c->sens.d_Fm.alloc(R.nF * n_par)); HIPCHK(c->sens.d_x.alloc((size_t)R.S * n_par * A.n_unk));
  return smallsignal_linearise(c, R.mode);
}

// The perturbed evaluations at the fixed operating point: F(p + h), F(p - h) (or F(p)) per parameter into c->sens.d_Fp / d_Fm, the
// step plan and dsrc into R.  want_gc: the launches also deliver G and C, into c->sens.d_Gp / d_Cp and d_Gm / d_Cm — one pair per sign, reused by
// every parameter — and hook(k, central) runs once both signs of parameter k are there (central == false: the minus side is the
// operating point's own G, C).  sign_hook(k, sign, a, src), optional: runs behind every single evaluation, in stream order and before
// the next sens_perturb overwrites the scratch tables of c->sens, with the perturbed argument set and source tables of that sign
// (ch_noise_sens rebuilds its source table from them); ch_dc_sens and ch_ac_sens pass none.
struct NoSignHook { int operator()(int, int, const NewtonArgs&, SourceTables) const { return CH_OK; } };
template <class Hook, class SignHook = NoSignHook>
static int sens_perturbed_evals(ch_circuit* c, int32_t n_par, const int32_t* slot_ids, bool want_gc, Hook&& hook, SensRun& R, SignHook&& sign_hook = SignHook()) {
  const int S = R.S, mode = R.mode; const size_t nF = R.nF;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  R.t_eval0 = hclock::now();
  R.plan = sens_plan_of(c, n_par, slot_ids, R.opt);
  R.dsrc.assign((size_t)n_par * S, 0.0);
  const SensPlan& P = R.plan; std::vector<double>& dsrc = R.dsrc;
  int rc = CH_OK;
  for (int k = 0; k < n_par; ++k) {
    const int id = P.slot[k], kind = P.kind[k], sa = P.src_of[k];
    const bool central = P.central[k] != 0;
    for (int sign = +1; sign >= (central ? -1 : +1); sign -= 2) {
      NewtonArgs a = c->nwt.base;
      TableOverride o;
      rc = sens_perturb(c, id, P.values(k, sign), o, a);
      if (rc != CH_OK) return rc;
      const SourceTables own = c->own_sources(), src{o.src_dc.empty() ? own.dc : &o.src_dc, o.src_par.empty() ? own.par : &o.src_par};
      double* dG = !want_gc ? c->ac.d_dumpA.p : sign > 0 ? c->sens.d_Gp.p : c->sens.d_Gm.p;
      double* dC = !want_gc ? nullptr : sign > 0 ? c->sens.d_Cp.p : c->sens.d_Cm.p;
      rc = smallsignal_eval(c, a, src, o.lds_extra_doubles * sizeof(double), mode, (sign > 0 ? c->sens.d_Fp.p : c->sens.d_Fm.p) + (size_t)k * nF, dG, dC);
      if (rc != CH_OK) return rc;
      rc = sign_hook(k, sign, a, src);
      if (rc != CH_OK) return rc;
      if (sign > 0 && P.is_src(k)) {
        // d(source value)/dp for the rows of known nodes: 1 where the slot IS the value, otherwise the same forward difference
        const int nsrc = (int)c->desc.src.size();
        for (int s = 0; s < S; ++s) {
          const size_t at = (size_t)(c->tab.Ssrc > 1 ? s : 0) * nsrc + sa;
          const bool is_value = kind == CH_SLOT_SRC_DC && (mode == 0 || c->desc.src[sa].kind == CH_SRC_DC);
          if (is_value) { dsrc[(size_t)k * S + s] = 1.0; continue; }
          const double vp = source_value(c->desc.src[sa], &(*src.par)[at * CH_SRC_NPAR], (*src.dc)[at], 0.0, mode);
          const double v0 = source_value(c->desc.src[sa], &(*own.par)[at * CH_SRC_NPAR], (*own.dc)[at], 0.0, mode);
          dsrc[(size_t)k * S + s] = (vp - v0) / P.h[(size_t)k * S + s];
        }
      }
      ++R.n_eval;
    }
    if (!central) HIPCHK(hipMemcpyAsync(c->sens.d_Fm.p + (size_t)k * nF, c->ac.d_dumpF0.p, nF * sizeof(double), hipMemcpyDeviceToDevice, c->ctx->stream));
    rc = hook(k, central);
    if (rc != CH_OK) return rc;
  }
  R.t_eval1 = hclock::now();
  return CH_OK;
}

// G · dx*/dp_k = -dF/dp_k for every parameter: results on the device (c->sens.d_x), in R.xs and — when asked for — expanded from
// unknown to MNA order in sens_out [S][n_par][n_mna] (what ch_dc_sens returns); R.fail != 0 when a G did not factor
static int sens_real_solves(ch_circuit* c, int32_t n_par, SensRun& R, double* sens_out) {
  const Analysis& A = c->desc.A;
  const int S = R.S;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  std::vector<int> zero(1, 0);
  HIPCHK(c->sens.d_den.upload(R.plan.den, c->ctx->stream)); HIPCHK(c->sens.d_skip.upload(R.skip, c->ctx->stream)); HIPCHK(c->sens.d_fail.upload(zero, c->ctx->stream));
  SensArgs a; std::memset(&a, 0, sizeof(a));
  a.bmeta = c->ac_bmeta(); a.G = c->ac.d_dumpG.p; a.Fp = c->sens.d_Fp.p; a.Fm = c->sens.d_Fm.p; a.den = c->sens.d_den.p; a.skip = c->sens.d_skip.p;
  if (!a.bmeta) return CH_ERR_DEVICE;
  a.f_stride = (long)R.nF; a.ds = R.ds; a.S = S; a.n_unk = A.n_unk; a.n_par = n_par; a.x_out = c->sens.d_x.p; a.fail = c->sens.d_fail.p;
  const int rc = launch_sens(c, a, R.nblk, n_par, R.nF, &R.solve_ms, &R.n_chunks, &R.n_solve_launches);
  if (rc != CH_OK) return rc;
  R.xs.assign((size_t)S * n_par * A.n_unk, 0.0);
  R.fail = 0;
  if (hipMemcpy(R.xs.data(), c->sens.d_x.p, R.xs.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&R.fail, c->sens.d_fail.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { c->set_err("DC sensitivities: reading the result back failed"); return CH_ERR_DEVICE; }
  if (sens_out) for (int s = 0; s < S; ++s) for (int k = 0; k < n_par; ++k)
    sens_expand_mna(A, R.skip[s] ? nullptr : &R.xs[((size_t)s * n_par + k) * A.n_unk], R.plan.src_of[k], R.dsrc[(size_t)k * S + s], sens_out + ((size_t)s * n_par + k) * A.n_mna);
  return CH_OK;
}

// The return code and message a sensitivity driver ends with: a singular G, then a singular G + jwC (complex_fail: the failure flag
// of the complex solves), otherwise what the operating point left
static int sens_outcome(ch_circuit* c, const char* analysis, const SensRun& R, int complex_fail) {
  if (R.fail) { c->set_err(std::string(analysis) + ": singular Jacobian G at the operating point"); return CH_ERR_SINGULAR; }
  if (complex_fail) { c->set_err(std::string(analysis) + ": singular small-signal matrix G + jwC"); return CH_ERR_SINGULAR; }
  if (R.rc_dc != CH_OK) c->set_err(R.dc_err);
  return R.rc_dc;
}

static int ch_dc_sens_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, double* x_out, double* sens_out,
                           int32_t* status_out, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  SensRun R;
  int rc = sens_check_args(c, "ch_dc_sens", n_par, slot_ids, sens_out, so, R.opt);
  if (rc != CH_OK) return rc;
  rc = sens_operating_point(c, o, "DC sensitivities", n_par, x_out, status_out, R);
  if (rc != CH_OK) return rc;
  rc = sens_perturbed_evals(c, n_par, slot_ids, false, [](int, bool) { return (int)CH_OK; }, R);   // right-hand sides: residual-only differences
  if (rc != CH_OK) return rc;
  rc = sens_real_solves(c, n_par, R, sens_out);
  if (rc != CH_OK) return rc;
  ch_stats& st = R.st;
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - R.t0).count();
  c->stats.fill(st);   // step_kernel_*: the evaluation launches behind the operating point
  st.device_seconds += R.solve_ms * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + R.n_solve_launches; st.nf += (int64_t)(R.n_eval + 1) * R.S; st.njacs += R.S; st.nfactors += (int64_t)R.nblk * R.n_chunks;
  st.nsolve += (int64_t)R.nblk * n_par;
  if (c->host_profile)
    std::fprintf(stderr, "[sens] operating point %.3f ms, %d evaluation launches %.3f ms (host wall), solve kernel %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3, R.n_eval,
                 std::chrono::duration<double>(R.t_eval1 - R.t_eval0).count() * 1e3, (double)R.solve_ms, st.wall_seconds * 1e3);
  if (stats) *stats = st;
  return sens_outcome(c, "DC sensitivities", R, 0);
}

// ---- AC parameter sensitivities (ch_ac_sens): Y dx/dp_k = -(dY/dp_k) x, Y = G + jwC.  dY/dp_k has two parts, both central (or exact
// forward) differences of the dense G, C dumps: the explicit one at the fixed operating point, out of the very perturbed evaluations
// the DC sensitivities make, and the state one, (dY/dx) s_k with s_k = dx*/dp_k, out of two evaluations with the circuit's own tables
// at x* +- eps_k s_k written to a scratch slot of the state ring.  acsens_rhs_kernel folds each difference into the right-hand sides
// as soon as it exists (one dense pair per sign, whatever n_par); acsens_solve_kernel factors Y once per frequency for all of them.
static int launch_acsens_rhs(ch_circuit* c, AcSensRhsArgs a, int k, bool minus_is_op, const double* den_k, int nblk, int n_freq, size_t r_stride, float* ms_acc) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  a.Gp = c->sens.d_Gp.p; a.Cp = c->sens.d_Cp.p;
  a.Gm = minus_is_op ? c->ac.d_dumpG.p : c->sens.d_Gm.p; a.Cm = minus_is_op ? c->ac.d_dumpC.p : c->sens.d_Cm.p;
  a.den = den_k; a.R = c->sens.d_R.p + (size_t)k * r_stride;
  if (ms_acc) HIPCHK(timed_begin(c));
  hipLaunchKernelGGL(acsens_rhs_kernel, dim3(nblk, (n_freq + ACSENS_FT - 1) / ACSENS_FT), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  if (ms_acc) HIPCHK(timed_end(c, ms_acc));   // profiling run: one synchronisation per launch
  return CH_OK;
}

// The launches of one frequency-chunked dense complex solve (acsens_solve_kernel, noisesens_solve_kernel) between the timing events;
// ny systems per frequency, `per` doubles of global workspace per system.  per == 0: a system lives in LDS and one launch takes
// every frequency, launch(0, n_freq, nullptr).  Otherwise one launch per chunk of frequencies whose workspace stays under the cap
// (dense_work_chunk), launch(f0, count, workspace).  who: the entry point, for the messages.  *ms_out (zero at the call) takes the event time.
template <class Launch>
static int launch_freq_chunks(ch_circuit* c, const std::string& who, int n_freq, int ny, size_t per, Launch&& launch, float* ms_out, int* n_launches) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  *n_launches = 0;
  HIPCHK(timed_begin(c));
  if (per == 0) {
    launch(0, n_freq, nullptr);
    HIPCHK(hipGetLastError());
    *n_launches = 1;
  } else {
    auto failed = [&]() { c->set_err(who + ": the dense complex solve failed on the device"); return (int)CH_ERR_DEVICE; };
    const int chunk = dense_work_chunk(per, ny, n_freq);
    ScopedWorkspace work;
    if (work.alloc((size_t)chunk * ny * per) != hipSuccess) { c->set_err(who + ": out of device memory for the dense complex LU workspace"); return CH_ERR_DEVICE; }
    for (int f0 = 0; f0 < n_freq; f0 += chunk) {
      launch(f0, std::min(chunk, n_freq - f0), work.p);
      if (hipGetLastError() != hipSuccess) return failed();
      *n_launches += 1;
    }
    if (hipStreamSynchronize(c->ctx->stream) != hipSuccess) return failed();
  }
  HIPCHK(timed_end(c, ms_out));
  return CH_OK;
}

// Y(w) X = R for every (frequency, block, sample): up to 96 unknowns one wavefront with factors and panel in LDS, above that the
// 256-thread variant on a global workspace, a chunk of frequencies per launch
static int launch_acsens(ch_circuit* c, AcSensSolveArgs& a, int n_freq, int nblk, int ds, int n_par, float* ms_out, int* n_launches) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  const bool in_lds = ds <= 96;
  size_t budget = 0;
  if (in_lds) HIPCHK(lds_budget_doubles((const void*)acsens_solve_kernel<64>, &budget));
  a.kp = in_lds ? acsens_panel_columns(ds, n_par, budget) : std::min(n_par, ACSENS_MAX_PANEL);
  if (a.kp < 1) { c->set_err("ch_ac_sens: the factors of a block do not fit the LDS"); return CH_ERR_INTERNAL; }
  const size_t lds = acsens_lds_doubles(ds, a.kp) * sizeof(double), per = in_lds ? 0 : acsens_work_doubles(ds, a.kp);
  a.work_per = (long)per;
  return launch_freq_chunks(c, "ch_ac_sens", n_freq, nblk, per, [&](int f0, int nf, double* work) {
    a.f0 = f0; a.work = work;
    if (in_lds) hipLaunchKernelGGL(acsens_solve_kernel<64>, dim3(nf, nblk), dim3(64), lds, st, a);
    else hipLaunchKernelGGL(acsens_solve_kernel<256>, dim3(nf, nblk), dim3(256), 0, st, a);
  }, ms_out, n_launches);
}

// ---- dY/dp_k as ch_ac_sens and ch_noise_sens form it.  accumulate(k, minus_is_op, den_k) folds the difference of the dumps in
// c->sens.d_Gp / d_Cp and d_Gm / d_Cm (minus_is_op: the operating point's own G, C) over the divisors den_k[S] into parameter k. ----
// the buffers of both terms: one pair of dense dumps per sign, the divisors and the state shifts
static int acsens_alloc_differences(ch_circuit* c, int n_par, const SensRun& R) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  HIPCHK(c->sens.d_Gp.alloc(R.nA)); HIPCHK(c->sens.d_Gm.alloc(R.nA)); HIPCHK(c->sens.d_Cp.alloc(R.nA)); HIPCHK(c->sens.d_Cm.alloc(R.nA));
  HIPCHK(c->sens.d_den_ac.alloc((size_t)n_par * R.S)); HIPCHK(c->sens.d_eps.alloc((size_t)n_par * R.S));
  return CH_OK;
}
// explicit term, the hook of sens_perturbed_evals: the divisors of parameter k go up, then the difference is folded in
template <class Accumulate>
static int acsens_explicit_term(ch_circuit* c, const SensRun& R, int k, bool central, Accumulate&& accumulate) {
  double* den_k = c->sens.d_den_ac.p + (size_t)k * R.S;
  if (hipMemcpyAsync(den_k, &R.plan.den[(size_t)k * R.S], R.S * sizeof(double), hipMemcpyHostToDevice, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  return accumulate(k, !central, den_k);
}
// State term: G, C at x* +- eps_k s_k (s_k = dx*/dp_k, in c->sens.d_x and R.xs) with the circuit's own tables, the shifted state in
// ring slot ACSENS_X_SLOT; skipped where G and C cannot depend on x.  after_eval(sign) runs behind each of the two evaluations of a
// parameter (ch_noise_sens rebuilds its source table at the shifted state), accumulate as above.  Leaves R.n_state and R.t_state0 / 1.
constexpr int ACSENS_X_SLOT = 2;   // the ring slot of the shifted state; MODE_EVAL writes its candidate to slot 1, slot 0 is the operating point
template <class AfterEval, class Accumulate>
static int acsens_state_term(ch_circuit* c, int n_par, SensRun& R, AfterEval&& after_eval, Accumulate&& accumulate) {
  const Analysis& A = c->desc.A;
  const int S = R.S, nu = A.n_unk;
  hipStream_t stream = c->ctx->stream;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  R.t_state0 = R.t_state1 = hclock::now();
  if (!acsens_state_dependent(A) || R.fail) return CH_OK;
  const double dv = R.opt.rel_step * 1.0;   // volts
  std::vector<double> eps((size_t)n_par * S, 0.0), den2((size_t)n_par * S, 1.0);
  for (int k = 0; k < n_par; ++k) for (int s = 0; s < S; ++s) {
    const double e = R.skip[s] ? 0.0 : acsens_state_eps(A, &R.xs[((size_t)s * n_par + k) * nu], dv);
    eps[(size_t)k * S + s] = e; if (e != 0.0) den2[(size_t)k * S + s] = 2.0 * e;
  }
  HIPCHK(c->sens.d_eps.upload(eps, stream)); HIPCHK(c->sens.d_den_ac.upload(den2, stream));
  HIPCHK(c->ac.d_dumpF.alloc(R.nF));   // the residual of the shifted evaluations is not used, but the launch writes it (ch_ac_sens has the buffer from ac_rhs)
  const long nxs = (long)S * nu;
  for (int k = 0; k < n_par; ++k) {
    bool any = false;
    for (int s = 0; s < S; ++s) any = any || eps[(size_t)k * S + s] != 0.0;
    if (!any) continue;
    for (int sign = +1; sign >= -1; sign -= 2) {
      hipLaunchKernelGGL(acsens_shift_kernel, dim3((unsigned)((nxs + 255) / 256)), dim3(256), 0, stream, c->nwt.d_X.p, c->nwt.base.slot_stride, ACSENS_X_SLOT,
                         (const double*)c->sens.d_x.p, k, (int)n_par, (const double*)(c->sens.d_eps.p + (size_t)k * S), (double)sign, nu, S);
      HIPCHK(hipGetLastError());
      int rc = smallsignal_eval(c, c->nwt.base, c->own_sources(), 0, R.mode, c->ac.d_dumpF.p, sign > 0 ? c->sens.d_Gp.p : c->sens.d_Gm.p, sign > 0 ? c->sens.d_Cp.p : c->sens.d_Cm.p, ACSENS_X_SLOT);
      if (rc == CH_OK) rc = after_eval(sign);
      if (rc != CH_OK) return rc;
      ++R.n_eval;
    }
    const int rc = accumulate(k, false, c->sens.d_den_ac.p + (size_t)k * S);
    if (rc != CH_OK) return rc;
    ++R.n_state;
  }
  R.t_state1 = hclock::now();
  return CH_OK;
}

// ch_ac_sens in two halves.  acsens_device_solve: the checks and every launch; it leaves x in c->ac.d_xac ([S][n_freq][n_unk][2]) and
// dx/dp in c->sens.d_xac_sens ([S][n_freq][n_par][n_unk][2]), in unknown order, and what the second half needs in an AcSensDevice.
// acsens_finish: the statistics and the return code.  ch_ac_sens reads back and expands between them; ch_ac_measure
// (ch_engine_fmeasure.hpp) measures the rows where they lie.
struct AcSensDevice {
  SensRun R; float csolve_ms = 0.0f, rhs_ms = 0.0f; int n_csolve = 0, n_rhs = 0;
};
static int acsens_device_solve(ch_circuit* c, const char* who, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq,
                               const double* freqs_hz, const void* sens_out, double* dc_sens_out, int32_t* status_out, AcSensDevice& D) {
  SensRun& R = D.R;
  const std::string w(who);
  int rc = sens_check_args(c, who, n_par, slot_ids, sens_out, so, R.opt);
  if (rc != CH_OK) return rc;
  if (n_freq < 1 || !freqs_hz) { c->set_err(w + ": at least one frequency"); return CH_ERR_INVALID; }
  rc = check_frequencies(c, n_freq, freqs_hz);
  if (rc != CH_OK) return rc;
  for (int k = 0; k < n_par; ++k) {   // the one slot that moves the AC right-hand side b
    const int id = slot_ids[k], sa = c->desc.slot_a[id];
    if (c->desc.slot_kind[id] != CH_SLOT_DEV_MULT || c->desc.dev[sa].kind != CH_DEV_I) continue;
    const int si = c->desc.dev[sa].ipar[0];
    if (si >= 0 && si < (int)c->desc.src.size() && c->desc.src[si].ac != 0.0) { c->set_err(w + ": the multiplier of an AC-driven current source is not a supported slot (it moves b)"); return CH_ERR_UNSUPPORTED; }
  }
  rc = sens_operating_point(c, o, "AC sensitivities", n_par, nullptr, status_out, R);
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  const int S = R.S, nblk = R.nblk, ds = R.ds, nu = A.n_unk;
  hipStream_t stream = c->ctx->stream;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  // ---- the small-signal solution x: the right-hand side and the solves of ch_ac, unchanged ----
  rc = ac_rhs(c, R.mode);
  if (rc != CH_OK) return rc;
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  const BlockMeta* bmeta = c->ac_bmeta();
  if (!bmeta) return CH_ERR_DEVICE;
  rc = ac_solve(c, bmeta, n_freq);   // (its failure flag is not read: a breakdown shows again in acsens_solve_kernel, which skips failed samples)
  if (rc != CH_OK) return rc;
  // ---- explicit term: every perturbed evaluation also leaves G+-, C+-, folded into R at once ----
  const size_t r_stride = (size_t)nblk * n_freq * ds * 2;
  rc = acsens_alloc_differences(c, n_par, R);
  if (rc != CH_OK) return rc;
  HIPCHK(c->sens.d_R.alloc(r_stride * n_par));
  HIPCHK(hipMemsetAsync(c->sens.d_R.p, 0, r_stride * n_par * sizeof(double), stream));
  std::vector<int> zero(1, 0);
  HIPCHK(c->sens.d_skip.upload(R.skip, stream));
  AcSensRhsArgs ra; std::memset(&ra, 0, sizeof(ra));
  ra.bmeta = bmeta; ra.skip = c->sens.d_skip.p; ra.x = c->ac.d_xac.p; ra.omega = c->ac.d_omega.p; ra.ds = ds; ra.S = S; ra.n_unk = nu; ra.n_freq = n_freq;
  float* rhs_acc = c->host_profile ? &D.rhs_ms : nullptr;
  auto accumulate = [&](int k, bool minus_is_op, const double* den_k) {
    ++D.n_rhs;
    return launch_acsens_rhs(c, ra, k, minus_is_op, den_k, nblk, n_freq, r_stride, rhs_acc);
  };
  rc = sens_perturbed_evals(c, n_par, slot_ids, true, [&](int k, bool central) { return acsens_explicit_term(c, R, k, central, accumulate); }, R);
  if (rc != CH_OK) return rc;
  // ---- s_k = dx*/dp_k (what ch_dc_sens returns) ----
  rc = sens_real_solves(c, n_par, R, dc_sens_out);
  if (rc != CH_OK) return rc;
  // ---- state term ----
  rc = acsens_state_term(c, n_par, R, [](int) { return (int)CH_OK; }, accumulate);
  if (rc != CH_OK) return rc;
  // ---- the complex solves ----
  const size_t nxs_out = (size_t)S * n_freq * n_par * nu * 2;
  HIPCHK(c->sens.d_xac_sens.alloc(nxs_out)); HIPCHK(c->sens.d_fail.upload(zero, stream));
  AcSensSolveArgs sa; std::memset(&sa, 0, sizeof(sa));
  sa.bmeta = bmeta; sa.G = c->ac.d_dumpG.p; sa.C = c->ac.d_dumpC.p; sa.R = c->sens.d_R.p; sa.omega = c->ac.d_omega.p; sa.skip = c->sens.d_skip.p;
  sa.ds = ds; sa.S = S; sa.n_unk = nu; sa.n_freq = n_freq; sa.n_par = n_par; sa.nblk = nblk; sa.x_out = c->sens.d_xac_sens.p; sa.fail = c->sens.d_fail.p;
  return launch_acsens(c, sa, n_freq, nblk, ds, n_par, &D.csolve_ms, &D.n_csolve);
}
// own_launches: the caller's kernels behind the solves; fail: the failure flag of the complex solves (c->sens.d_fail), read by the caller
static int acsens_finish(ch_circuit* c, AcSensDevice& D, int n_par, int n_freq, int own_launches, int fail, ch_stats* stats) {
  SensRun& R = D.R;
  const int S = R.S, nblk = R.nblk;
  ch_stats& st = R.st;
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - R.t0).count();
  c->stats.fill(st);
  st.device_seconds += (R.solve_ms + D.csolve_ms) * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + R.n_solve_launches + D.n_csolve + D.n_rhs + 2 * R.n_state + 2 + own_launches;
  st.nf += (int64_t)(R.n_eval + 2) * S; st.njacs += (int64_t)(R.n_eval + 1) * S;
  st.nfactors += (int64_t)nblk * R.n_chunks + (int64_t)2 * nblk * n_freq; st.nsolve += (int64_t)nblk * n_par + (int64_t)nblk * n_freq * (n_par + 1);
  if (c->host_profile)
    std::fprintf(stderr, "[acsens] operating point %.3f ms, explicit evaluations %.3f ms, state evaluations (%d parameters) %.3f ms (host wall, rhs launches included), "
                 "rhs kernel %d launches %.3f ms, real solve %.3f ms, complex solve %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3,
                 std::chrono::duration<double>(R.t_eval1 - R.t_eval0).count() * 1e3, R.n_state, std::chrono::duration<double>(R.t_state1 - R.t_state0).count() * 1e3,
                 D.n_rhs, (double)D.rhs_ms, (double)R.solve_ms, (double)D.csolve_ms, st.wall_seconds * 1e3);
  if (stats) *stats = st;
  return sens_outcome(c, "AC sensitivities", R, fail);
}

static int ch_ac_sens_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq, const double* freqs_hz,
                           double* x_ac_out, double* dc_sens_out, double* sens_out, int32_t* status_out, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  AcSensDevice D;
  const int rc = acsens_device_solve(c, "ch_ac_sens", o, n_par, slot_ids, so, n_freq, freqs_hz, sens_out, dc_sens_out, status_out, D);
  if (rc != CH_OK) return rc;
  const SensRun& R = D.R;
  const Analysis& A = c->desc.A;
  const int S = R.S, nu = A.n_unk, nm = A.n_mna;
  const size_t nx = (size_t)S * n_freq * nu * 2, nxs_out = nx * n_par;
  std::vector<double> xs(nx), zs(nxs_out);
  int fail = 0;
  if (hipMemcpy(xs.data(), c->ac.d_xac.p, nx * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(zs.data(), c->sens.d_xac_sens.p, nxs_out * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&fail, c->sens.d_fail.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { c->set_err("AC sensitivities: reading the result back failed"); return CH_ERR_DEVICE; }
  // ---- unknown order -> MNA order ----
  for (int s = 0; s < S; ++s) for (int f = 0; f < n_freq; ++f) {
    const size_t sf = (size_t)s * n_freq + f;
    if (x_ac_out) acsens_expand_mna(A, R.skip[s] ? nullptr : &xs[sf * nu * 2], x_ac_out + sf * nm * 2);
    for (int k = 0; k < n_par; ++k) acsens_expand_mna(A, R.skip[s] ? nullptr : &zs[(sf * n_par + k) * nu * 2], sens_out + (sf * n_par + k) * nm * 2);
  }
  return acsens_finish(c, D, n_par, n_freq, 0, fail, stats);
}
}  // extern "C++"
