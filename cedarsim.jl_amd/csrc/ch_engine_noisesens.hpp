// ch_engine_noisesens.hpp — noise PSD parameter sensitivities by the direct method on the adjoint system (ch_noise_sens).
// With Y = G + jwC, Y^T y = e_out and S = sum_e |dy_e|^2 pwr_e / f^ex_e over the output block's source table:
//   Y^T dy_k = -(dY/dp_k)^T y,   dS/dp_k = sum_e [ 2 Re(conj(dy_e) d(dy)_{k,e}) pwr_e + |dy_e|^2 dpwr_{k,e} ] / f^ex_e.
// dY/dp_k is the matrix ch_ac_sens forms (explicit difference of the perturbed evaluations at the fixed operating point plus the
// state difference at x* +- eps_k s_k); dpwr_k is the same pair of differences of the source table, built by the two table kernels
// of ch_noise / ch_noise_ex with the perturbed tables, then with the own tables at the shifted states.  The front half — operating
// point, perturbed evaluations, real solves — is ch_engine_sens.hpp's, the table and the PSD launch ch_engine_ac.hpp's; the HIP-free
// half is ch_noisesens_host.hpp, the kernels are in ch_noisesens_kernels.hpp.  Included by ch_engine.hip behind ch_engine_sens.hpp.
#pragma once

extern "C++" {

// Y^T(w) solves of the output block, one system per (frequency, sample): n_par == 0 stores y, otherwise dS/dp of every parameter.
// Up to 96 unknowns one wavefront with factors, y and a panel in LDS; above that the 256-thread variant on a global workspace, a
// chunk of frequencies per launch.
static int launch_noisesens(ch_circuit* c, NoiseSensSolveArgs& a, int n_freq, int S, int nc, int n_par, float* ms_out, int* n_launches) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  *n_launches = 0;
  HIPCHK(hipEventRecord(c->nwt.ev0, st));
  if (nc <= 96) {
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, (const void*)noisesens_solve_kernel<64>));
    const size_t budget = (size_t)((160 * 1024 - (int)fa.sharedSizeBytes) & ~255) / sizeof(double);   // what raise_lds_ceilings granted
    const int kp = noisesens_panel_columns(nc, n_par, budget);
    if (kp < 0) { c->set_err("ch_noise_sens: the factors of the output block do not fit the LDS"); return CH_ERR_INTERNAL; }
    a.kp = kp; a.f0 = 0; a.work = nullptr; a.work_per = 0;
    hipLaunchKernelGGL(noisesens_solve_kernel<64>, dim3(n_freq, S), dim3(64), noisesens_lds_doubles(nc, kp) * sizeof(double), st, a);
    HIPCHK(hipGetLastError());
    *n_launches = 1;
  } else {
    const int kp = noisesens_work_columns(n_par);
    const size_t per = noisesens_work_doubles(nc, kp);
    const int chunk = noisesens_freq_chunk(nc, kp, S, n_freq);
    auto failed = [&]() { c->set_err("ch_noise_sens: the dense complex solve failed on the device"); return (int)CH_ERR_DEVICE; };
    ScopedWorkspace work;
    if (work.alloc((size_t)chunk * S * per) != hipSuccess) { c->set_err("ch_noise_sens: out of device memory for the dense complex LU workspace"); return CH_ERR_DEVICE; }
    for (int f0 = 0; f0 < n_freq; f0 += chunk) {
      a.kp = kp; a.f0 = f0; a.work = work.p; a.work_per = (long)per;
      hipLaunchKernelGGL(noisesens_solve_kernel<256>, dim3(std::min(chunk, n_freq - f0), S), dim3(256), 0, st, a);
      if (hipGetLastError() != hipSuccess) return failed();
      *n_launches += 1;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return failed();
  }
  HIPCHK(hipEventRecord(c->nwt.ev1, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(ms_out, c->nwt.ev0, c->nwt.ev1));
  return CH_OK;
}

static int ch_noise_sens_impl(ch_circuit* c, const ch_dc_opts* o, const ch_noise_opts* no, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t out_kind,
                              int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out, double* dpsd_out, double* dc_sens_out, int32_t* status_out,
                              ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  SensRun R;
  int rc = sens_check_args(c, "ch_noise_sens", n_par, slot_ids, dpsd_out, so, R.opt);
  if (rc != CH_OK) return rc;
  if (!psd_out) { c->set_err("ch_noise_sens: psd_out is required"); return CH_ERR_INVALID; }
  if (n_freq < 1 || !freqs_hz) { c->set_err("ch_noise_sens: at least one frequency"); return CH_ERR_INVALID; }
  rc = check_frequencies(c, n_freq, freqs_hz);
  if (rc != CH_OK) return rc;
  const int mos_noise = (no && no->mos_noise) ? 1 : 0;
  c->ac.last_noise.valid = false;
  int u_out = -1;
  rc = noise_output_unknown(c, out_kind, out_index, u_out);
  if (rc != CH_OK) return rc;
  rc = sens_operating_point(c, o, "noise sensitivities", n_par, nullptr, status_out, R);
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  const int S = R.S, nblk = R.nblk, ds = R.ds, nu = A.n_unk;
  const size_t nA = R.nA;
  hipStream_t stream = c->ctx->stream;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  auto finish = [&](ch_stats& st) { st.wall_seconds = std::chrono::duration<double>(hclock::now() - R.t0).count(); if (stats) *stats = st; };
  if (u_out < 0) {   // a node held by ideal sources carries no noise, whatever the parameters; a sample without an operating point is still not served
    for (int s = 0; s < S; ++s) {
      std::fill(psd_out + (size_t)s * n_freq, psd_out + (size_t)(s + 1) * n_freq, R.skip[s] ? CH_NAN : 0.0);
      std::fill(dpsd_out + (size_t)s * n_freq * n_par, dpsd_out + (size_t)(s + 1) * n_freq * n_par, R.skip[s] ? CH_NAN : 0.0);
    }
    if (dc_sens_out) {
      rc = sens_perturbed_evals(c, n_par, slot_ids, false, [](int, bool) { return (int)CH_OK; }, R);
      if (rc == CH_OK) rc = sens_real_solves(c, n_par, R);
      if (rc != CH_OK) return rc;
      sens_expand_all(c, n_par, R, dc_sens_out);
    }
    c->stats.fill(R.st);
    finish(R.st);
    if (R.fail) { c->set_err("noise sensitivities: singular Jacobian G at the operating point"); return CH_ERR_SINGULAR; }
    if (R.rc_dc != CH_OK) c->set_err(R.dc_err);
    return R.rc_dc;
  }
  const int comp = c->ac_comp_of(u_out), ncb = c->ac_nc(comp), n_tab = c->ac_ndev(comp) * va::MAX_NOISE;
  const size_t nT = (size_t)S * n_tab;
  // ---- the source table at x* and the PSD: the launches of ch_noise / ch_noise_ex ----
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  NoiseTabArgs t0;
  rc = noise_table_setup(c, R.mode, comp, n_freq, t0); if (rc != CH_OK) return rc;
  rc = noise_table_launch(c, t0, mos_noise); if (rc != CH_OK) return rc;
  AcArgs pa;
  rc = noise_solve_args(c, comp, u_out, n_freq, pa); if (rc != CH_OK) return rc;
  rc = launch_ac(c, pa, n_freq, S, ds); if (rc != CH_OK) return rc;
  // ---- y for every (sample, frequency): the solve kernel without parameters ----
  NoiseSensitivity& N = c->nsens;
  const size_t r_stride = (size_t)S * n_freq * ds * 2;
  std::vector<int> zero(1, 0), zeros_k(n_par, 0);
  HIPCHK(N.d_y.alloc((size_t)S * n_freq * ncb * 2)); HIPCHK(N.d_R.alloc(r_stride * n_par)); HIPCHK(N.d_dpwr.alloc(nT * n_par)); HIPCHK(N.d_dpsd.alloc((size_t)S * n_freq * n_par));
  HIPCHK(N.d_pwr_p.alloc(nT)); HIPCHK(N.d_pwr_m.alloc(nT)); HIPCHK(N.d_ex_p.alloc(nT)); HIPCHK(N.d_ex_m.alloc(nT)); HIPCHK(N.d_na.alloc(nT)); HIPCHK(N.d_nb.alloc(nT));
  HIPCHK(c->sens.d_Gp.alloc(nA)); HIPCHK(c->sens.d_Gm.alloc(nA)); HIPCHK(c->sens.d_Cp.alloc(nA)); HIPCHK(c->sens.d_Cm.alloc(nA));
  HIPCHK(c->sens.d_den_ac.alloc((size_t)n_par * S)); HIPCHK(c->sens.d_eps.alloc((size_t)n_par * S));
  HIPCHK(hipMemsetAsync(N.d_R.p, 0, r_stride * n_par * sizeof(double), stream)); HIPCHK(hipMemsetAsync(N.d_dpwr.p, 0, nT * n_par * sizeof(double), stream));
  HIPCHK(c->sens.d_skip.upload(R.skip, stream)); HIPCHK(c->sens.d_fail.upload(zero, stream)); HIPCHK(N.d_ex_moved.upload(zeros_k, stream));
  NoiseSensSolveArgs sa; std::memset(&sa, 0, sizeof(sa));
  sa.bmeta = pa.bmeta; sa.G = c->ac.d_dumpG.p; sa.C = c->ac.d_dumpC.p; sa.R = N.d_R.p; sa.omega = c->ac.d_omega.p; sa.skip = c->sens.d_skip.p;
  sa.ds = ds; sa.S = S; sa.n_freq = n_freq; sa.n_par = 0; sa.comp = comp; sa.row_out = pa.row_out; sa.n_tab = n_tab;
  sa.na = c->ac.d_noise_a.p; sa.nb = c->ac.d_noise_b.p; sa.pwr = c->ac.d_noise_pwr.p; sa.ex = c->ac.d_noise_exp.p; sa.dpwr = N.d_dpwr.p;
  sa.y_out = N.d_y.p; sa.dpsd_out = N.d_dpsd.p; sa.fail = c->sens.d_fail.p;
  float y_ms = 0.0f, solve_ms = 0.0f; int n_ysolve = 0, n_csolve = 0;
  rc = launch_noisesens(c, sa, n_freq, S, ncb, 0, &y_ms, &n_ysolve);
  if (rc != CH_OK) return rc;
  // ---- one difference of dumps into R_k, one difference of tables into dpwr_k ----
  NoiseSensRhsArgs ra; std::memset(&ra, 0, sizeof(ra));
  ra.bmeta = pa.bmeta; ra.skip = c->sens.d_skip.p; ra.y = N.d_y.p; ra.omega = c->ac.d_omega.p; ra.ds = ds; ra.S = S; ra.n_freq = n_freq; ra.comp = comp;
  int n_small = 0;   // launches of the rhs, dpwr and table kernels
  auto accumulate = [&](int k, bool minus_is_op, const double* den_k) -> int {
    NoiseSensRhsArgs b = ra;
    b.Gp = c->sens.d_Gp.p; b.Cp = c->sens.d_Cp.p; b.Gm = minus_is_op ? c->ac.d_dumpG.p : c->sens.d_Gm.p; b.Cm = minus_is_op ? c->ac.d_dumpC.p : c->sens.d_Cm.p;
    b.den = den_k; b.R = N.d_R.p + (size_t)k * r_stride;
    hipLaunchKernelGGL(noisesens_rhs_kernel, dim3(S, (n_freq + ACSENS_FT - 1) / ACSENS_FT, (ncb + 63) / 64), dim3(64), 0, stream, b);
    HIPCHK(hipGetLastError());
    NoiseSensDpwrArgs d; std::memset(&d, 0, sizeof(d));
    d.pwr_p = N.d_pwr_p.p; d.ex_p = N.d_ex_p.p; d.pwr_m = minus_is_op ? c->ac.d_noise_pwr.p : N.d_pwr_m.p; d.ex_m = minus_is_op ? c->ac.d_noise_exp.p : N.d_ex_m.p;
    d.ex0 = c->ac.d_noise_exp.p; d.den = den_k; d.skip = c->sens.d_skip.p; d.dpwr = N.d_dpwr.p + (size_t)k * nT; d.ex_moved = N.d_ex_moved.p + k; d.S = S; d.n_tab = n_tab;
    if (nT > 0) hipLaunchKernelGGL(noisesens_dpwr_kernel, dim3((unsigned)((nT + 255) / 256)), dim3(256), 0, stream, d);
    HIPCHK(hipGetLastError());
    n_small += 2;
    return CH_OK;
  };
  // the source table with the tables of `a` and the sources `src` at the state X, into the scratch of `sign`
  const std::vector<double>& npar_own = c->ac.mos_npar_host;   // what launch_mos_noise built and uploaded for the operating point's table
  std::vector<double> sv_h, kv_h;
  auto build_table = [&](const NewtonArgs& a, SourceTables src, const double* X, int sign, const double* npar) -> int {
    c->eval_sources(0.0, R.mode, sv_h, kv_h, src);
    HIPCHK(N.d_kv.upload(kv_h, stream));
    NoiseTabArgs t = t0;
    t.dcls_local = a.dcls_local; t.dpar = a.dpar; t.dmult = a.dmult; t.vapar = a.vapar; t.temp_s = a.temp_s; t.gmin_s = a.gmin_s; t.X = X; t.kv = N.d_kv.p;
    t.na = N.d_na.p; t.nb = N.d_nb.p; t.pwr = sign > 0 ? N.d_pwr_p.p : N.d_pwr_m.p; t.ex = sign > 0 ? N.d_ex_p.p : N.d_ex_m.p;
    n_small += 1 + mos_noise;
    return noise_table_launch(c, t, mos_noise, a.dcls, a.mosp, npar);
  };
  rc = sens_perturbed_evals(c, n_par, slot_ids, true, [&](int k, bool central) {
    if (hipMemcpyAsync(c->sens.d_den_ac.p + (size_t)k * S, &R.den[(size_t)k * S], S * sizeof(double), hipMemcpyHostToDevice, stream) != hipSuccess) return (int)CH_ERR_DEVICE;
    return accumulate(k, !central, c->sens.d_den_ac.p + (size_t)k * S);
  }, R, [&](int k, int sign, const NewtonArgs& a, SourceTables src) {
    const double* npar = c->ac.d_mos_npar.p;
    if (mos_noise && a.n_mos_cls == c->tab.n_cls + 1) {   // the slot is an instance parameter of a MOSFET, which runs on class n_cls: one more row for it
      const int hd = c->desc.slot_a[slot_ids[k]];
      const int m = (int)(std::find(A.mos_hdev.begin(), A.mos_hdev.end(), hd) - A.mos_hdev.begin());
      const std::vector<double> ext = noisesens_npar_extra_row(npar_own, c->tab.n_cls, CH_B4N_NPAR, m < (int)A.mos_hdev.size() ? c->tab.mos_cls[m] : -1);
      if (ext.empty()) { c->set_err("ch_noise_sens: no MOSFET class behind the perturbed instance"); return (int)CH_ERR_INTERNAL; }
      if (N.d_npar.upload(ext, stream) != hipSuccess) return (int)CH_ERR_DEVICE;
      npar = N.d_npar.p;
    }
    return build_table(a, src, c->nwt.d_X.p, sign, npar);
  });
  if (rc != CH_OK) return rc;
  // ---- s_k = dx*/dp_k (what ch_dc_sens returns) ----
  rc = sens_real_solves(c, n_par, R);
  if (rc != CH_OK) return rc;
  if (dc_sens_out) sens_expand_all(c, n_par, R, dc_sens_out);
  // ---- state term: G, C and the source table at x* +- eps_k s_k with the circuit's own tables ----
  const auto t_state0 = hclock::now();
  int n_state = 0;
  if (acsens_state_dependent(A) && !R.fail) {
    const double dv = R.opt.rel_step * 1.0;   // volts
    std::vector<double> eps((size_t)n_par * S, 0.0), den2((size_t)n_par * S, 1.0);
    for (int k = 0; k < n_par; ++k) for (int s = 0; s < S; ++s) {
      const double e = R.skip[s] ? 0.0 : acsens_state_eps(A, &R.xs[((size_t)s * n_par + k) * nu], dv);
      eps[(size_t)k * S + s] = e; if (e != 0.0) den2[(size_t)k * S + s] = 2.0 * e;
    }
    HIPCHK(c->sens.d_eps.upload(eps, stream)); HIPCHK(c->sens.d_den_ac.upload(den2, stream));
    HIPCHK(c->ac.d_dumpF.alloc(R.nF));   // the residual of the shifted evaluations is not used, but the launch writes it (ch_ac_sens has the buffer from ac_rhs)
    const long nxs = (long)S * nu;
    const double* Xs = c->nwt.d_X.p + (size_t)ACSENS_X_SLOT * c->nwt.base.slot_stride;
    for (int k = 0; k < n_par; ++k) {
      bool any = false;
      for (int s = 0; s < S; ++s) any = any || eps[(size_t)k * S + s] != 0.0;
      if (!any) continue;
      for (int sign = +1; sign >= -1; sign -= 2) {
        hipLaunchKernelGGL(acsens_shift_kernel, dim3((unsigned)((nxs + 255) / 256)), dim3(256), 0, stream, c->nwt.d_X.p, c->nwt.base.slot_stride, ACSENS_X_SLOT,
                           (const double*)c->sens.d_x.p, k, (int)n_par, (const double*)(c->sens.d_eps.p + (size_t)k * S), (double)sign, nu, S);
        HIPCHK(hipGetLastError());
        rc = smallsignal_eval(c, c->nwt.base, c->own_sources(), 0, R.mode, c->ac.d_dumpF.p, sign > 0 ? c->sens.d_Gp.p : c->sens.d_Gm.p, sign > 0 ? c->sens.d_Cp.p : c->sens.d_Cm.p, ACSENS_X_SLOT);
        if (rc != CH_OK) return rc;
        rc = build_table(c->nwt.base, c->own_sources(), Xs, sign, c->ac.d_mos_npar.p);
        if (rc != CH_OK) return rc;
        ++R.n_eval;
      }
      rc = accumulate(k, false, c->sens.d_den_ac.p + (size_t)k * S);
      if (rc != CH_OK) return rc;
      ++n_state;
    }
  }
  const auto t_state1 = hclock::now();
  // ---- the transposed solves with every parameter, and the reduction over the table ----
  sa.n_par = n_par;
  rc = launch_noisesens(c, sa, n_freq, S, ncb, n_par, &solve_ms, &n_csolve);
  if (rc != CH_OK) return rc;
  const size_t nd = (size_t)S * n_freq * n_par;
  std::vector<int> ex_moved(n_par, 0);
  int fail = 0, mfail = 0;
  bool okc = hipMemcpy(psd_out, c->ac.d_psd.p, (size_t)S * n_freq * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(dpsd_out, N.d_dpsd.p, nd * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(ex_moved.data(), N.d_ex_moved.p, n_par * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(&fail, c->sens.d_fail.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  if (okc && mos_noise) okc = hipMemcpy(&mfail, c->ac.d_mos_fail.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  if (!okc) { c->set_err("noise sensitivities: reading the result back failed"); return CH_ERR_DEVICE; }
  for (int s = 0; s < S; ++s) {
    if (R.skip[s]) {   // not served: the operating point failed
      std::fill(psd_out + (size_t)s * n_freq, psd_out + (size_t)(s + 1) * n_freq, CH_NAN);
      std::fill(dpsd_out + (size_t)s * n_freq * n_par, dpsd_out + (size_t)(s + 1) * n_freq * n_par, CH_NAN);
    } else for (int f = 0; f < n_freq; ++f) if (std::isnan(psd_out[(size_t)s * n_freq + f])) fail = 1;   // (ac_block_kernel's own flag also counts the samples not served)
  }
  ch_stats& st = R.st;
  c->stats.fill(st);
  st.device_seconds += (R.solve_ms + y_ms + solve_ms) * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + R.n_solve_launches + n_ysolve + n_csolve + n_small + 2 * n_state + 2 + mos_noise;
  st.nf += (int64_t)(R.n_eval + 1) * S; st.njacs += (int64_t)(R.n_eval + 1) * S;
  st.nfactors += (int64_t)nblk * R.n_chunks + (int64_t)3 * S * n_freq; st.nsolve += (int64_t)nblk * n_par + (int64_t)S * n_freq * (n_par + 3);
  finish(st);
  if (c->host_profile)
    std::fprintf(stderr, "[noisesens] operating point %.3f ms, explicit evaluations %.3f ms, state evaluations (%d parameters) %.3f ms (host wall, table, rhs and dpwr launches included), "
                 "%d small launches, real solve %.3f ms, y solve %.3f ms, parameter solve %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3,
                 std::chrono::duration<double>(R.t_eval1 - R.t_eval0).count() * 1e3, n_state, std::chrono::duration<double>(t_state1 - t_state0).count() * 1e3,
                 n_small, (double)R.solve_ms, (double)y_ms, (double)solve_ms, st.wall_seconds * 1e3);
  if (mfail) { c->set_err("MOSFET noise: a BSIM4 card without an intrinsic charge model (capmod 0 or xpart < 0) has no inversion charge to take the channel noise from"); return CH_ERR_UNSUPPORTED; }
  for (int k = 0; k < n_par; ++k) if (ex_moved[k]) {
    c->set_err("ch_noise_sens: slot " + std::to_string(slot_ids[k]) + " moves the exponent of a flicker source, which is not differentiated");
    return CH_ERR_UNSUPPORTED;
  }
  if (R.fail) { c->set_err("noise sensitivities: singular Jacobian G at the operating point"); return CH_ERR_SINGULAR; }
  if (fail) { c->set_err("noise sensitivities: singular small-signal matrix G + jwC"); return CH_ERR_SINGULAR; }
  if (R.rc_dc != CH_OK) c->set_err(R.dc_err);
  return R.rc_dc;
}
}  // extern "C++"
