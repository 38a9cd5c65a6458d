// ch_engine_noisesens.hpp — noise PSD parameter sensitivities by the direct method on the adjoint system (ch_noise_sens).
// With Y = G + jwC, Y^T y = e_out and S = sum_e |dy_e|^2 pwr_e / f^ex_e over the output block's source table:
//   Y^T dy_k = -(dY/dp_k)^T y,   dS/dp_k = sum_e [ 2 Re(conj(dy_e) d(dy)_{k,e}) pwr_e + |dy_e|^2 dpwr_{k,e} ] / f^ex_e.
// dY/dp_k is the matrix ch_ac_sens forms (explicit difference of the perturbed evaluations at the fixed operating point plus the
// state difference at x* +- eps_k s_k); dpwr_k is the same pair of differences of the source table, built by the two table kernels
// of ch_noise / ch_noise_ex with the perturbed tables, then with the own tables at the shifted states.  The front half — operating
// point, perturbed evaluations, real solves — the two passes over the parameters (acsens_explicit_term, acsens_state_term), the chunk
// launcher and the outcome rule are ch_engine_sens.hpp's, the table and the PSD launch ch_engine_ac.hpp's; the HIP-free half is
// ch_noisesens_host.hpp, the kernels are in ch_noisesens_kernels.hpp.  ch_noise_sens_impl runs the numbered steps below over one
// NoiseSensRun.  Included by ch_engine.hip behind ch_engine_sens.hpp.
#pragma once

extern "C++" {

// Y^T(w) solves of the output block, one system per (frequency, sample): n_par == 0 stores y, otherwise dS/dp of every parameter.
// Up to 96 unknowns one wavefront with factors, y and a panel in LDS; above that the 256-thread variant on a global workspace, a
// chunk of frequencies per launch.
static int launch_noisesens(ch_circuit* c, NoiseSensSolveArgs& a, int n_freq, int S, int nc, int n_par, float* ms_out, int* n_launches) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  const bool in_lds = nc <= 96;
  size_t budget = 0;
  if (in_lds) HIPCHK(lds_budget_doubles((const void*)noisesens_solve_kernel<64>, &budget));
  a.kp = in_lds ? noisesens_panel_columns(nc, n_par, budget) : noisesens_work_columns(n_par);
  if (a.kp < 0) { c->set_err("ch_noise_sens: the factors of the output block do not fit the LDS"); return CH_ERR_INTERNAL; }
  const size_t per = in_lds ? 0 : noisesens_work_doubles(nc, a.kp);
  a.work_per = (long)per;   // (the chunk of frequencies is noisesens_freq_chunk's: dense_work_chunk over S systems of `per` doubles)
  return launch_freq_chunks(c, "ch_noise_sens", n_freq, S, per, [&](int f0, int nf, double* work) {
    a.f0 = f0; a.work = work;
    if (in_lds) hipLaunchKernelGGL(noisesens_solve_kernel<64>, dim3(nf, S), dim3(64), noisesens_lds_doubles(nc, a.kp) * sizeof(double), st, a);
    else hipLaunchKernelGGL(noisesens_solve_kernel<256>, dim3(nf, S), dim3(256), 0, st, a);
  }, ms_out, n_launches);
}

// ch_noise_sens in named steps over one record: what a step leaves for the next ones is here, the rest is in its signature
struct NoiseSensRun : SensRun {
  int mos_noise = 0, u_out = -1, comp = 0, ncb = 0, n_tab = 0; size_t nT = 0, r_stride = 0;   // output unknown and block; its table [S][n_tab]
  NoiseTabArgs tab0; AcArgs pa; NoiseSensSolveArgs sa; NoiseSensRhsArgs ra;                    // the table at x*, the PSD solve, the y / parameter solves, the rhs
  std::vector<double> sv_h, kv_h;                                                            // scratch of the table builds
  float y_ms = 0.0f, psolve_ms = 0.0f; int n_ysolve = 0, n_csolve = 0, n_small = 0;   // n_small: launches of the rhs, dpwr and table kernels
};

// 1. the arguments, before anything is computed; the output unknown (-1: held by ideal sources)
static int noisesens_check(ch_circuit* c, const ch_noise_opts* no, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t out_kind, int32_t out_index,
                           int32_t n_freq, const double* freqs_hz, const double* psd_out, const double* dpsd_out, NoiseSensRun& N) {
  int rc = sens_check_args(c, "ch_noise_sens", n_par, slot_ids, dpsd_out, so, N.opt);
  if (rc != CH_OK) return rc;
  if (!psd_out) { c->set_err("ch_noise_sens: psd_out is required"); return CH_ERR_INVALID; }
  if (n_freq < 1 || !freqs_hz) { c->set_err("ch_noise_sens: at least one frequency"); return CH_ERR_INVALID; }
  rc = check_frequencies(c, n_freq, freqs_hz);
  if (rc != CH_OK) return rc;
  N.mos_noise = (no && no->mos_noise) ? 1 : 0;
  c->ac.last_noise.valid = false;
  return noise_output_unknown(c, out_kind, out_index, N.u_out);
}

// 2. a node held by ideal sources carries no noise, whatever the parameters; a sample without an operating point is still not served
static int noisesens_held_output(ch_circuit* c, int32_t n_par, const int32_t* slot_ids, int32_t n_freq, double* psd_out, double* dpsd_out, double* dc_sens_out, NoiseSensRun& N,
                                 ch_stats* stats) {
  for (int s = 0; s < N.S; ++s) {
    std::fill(psd_out + (size_t)s * n_freq, psd_out + (size_t)(s + 1) * n_freq, N.skip[s] ? CH_NAN : 0.0);
    std::fill(dpsd_out + (size_t)s * n_freq * n_par, dpsd_out + (size_t)(s + 1) * n_freq * n_par, N.skip[s] ? CH_NAN : 0.0);
  }
  if (dc_sens_out) {
    int rc = sens_perturbed_evals(c, n_par, slot_ids, false, [](int, bool) { return (int)CH_OK; }, N);
    if (rc == CH_OK) rc = sens_real_solves(c, n_par, N, dc_sens_out);
    if (rc != CH_OK) return rc;
  }
  c->stats.fill(N.st);
  N.st.wall_seconds = std::chrono::duration<double>(hclock::now() - N.t0).count();
  if (stats) *stats = N.st;
  return sens_outcome(c, "noise sensitivities", N, 0);
}

// 3. the source table at x* and the PSD (the launches of ch_noise / ch_noise_ex), the buffers, then y for every (sample, frequency):
//    the solve kernel without parameters
static int noisesens_table_and_y(ch_circuit* c, int32_t n_par, int32_t n_freq, const double* freqs_hz, NoiseSensRun& N) {
  const int S = N.S, ds = N.ds;
  hipStream_t stream = c->ctx->stream;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  N.comp = c->ac_comp_of(N.u_out); N.ncb = c->ac_nc(N.comp); N.n_tab = c->ac_ndev(N.comp) * va::MAX_NOISE;
  N.nT = (size_t)S * N.n_tab; N.r_stride = (size_t)S * n_freq * ds * 2;
  const size_t nT = N.nT;
  int rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  rc = noise_table_setup(c, N.mode, N.comp, n_freq, N.tab0); if (rc != CH_OK) return rc;
  rc = noise_table_launch(c, N.tab0, N.mos_noise); if (rc != CH_OK) return rc;
  rc = noise_solve_args(c, N.comp, N.u_out, n_freq, N.pa); if (rc != CH_OK) return rc;
  rc = launch_ac(c, N.pa, n_freq, S, ds); if (rc != CH_OK) return rc;
  NoiseSensitivity& B = c->nsens;
  std::vector<int> zero(1, 0), zeros_k(n_par, 0);
  HIPCHK(B.d_y.alloc((size_t)S * n_freq * N.ncb * 2)); HIPCHK(B.d_R.alloc(N.r_stride * n_par)); HIPCHK(B.d_dpwr.alloc(nT * n_par)); HIPCHK(B.d_dpsd.alloc((size_t)S * n_freq * n_par));
  HIPCHK(B.d_pwr_p.alloc(nT)); HIPCHK(B.d_pwr_m.alloc(nT)); HIPCHK(B.d_ex_p.alloc(nT)); HIPCHK(B.d_ex_m.alloc(nT)); HIPCHK(B.d_na.alloc(nT)); HIPCHK(B.d_nb.alloc(nT));
  rc = acsens_alloc_differences(c, n_par, N);
  if (rc != CH_OK) return rc;
  HIPCHK(hipMemsetAsync(B.d_R.p, 0, N.r_stride * n_par * sizeof(double), stream)); HIPCHK(hipMemsetAsync(B.d_dpwr.p, 0, nT * n_par * sizeof(double), stream));
  HIPCHK(c->sens.d_skip.upload(N.skip, stream)); HIPCHK(c->sens.d_fail.upload(zero, stream)); HIPCHK(B.d_ex_moved.upload(zeros_k, stream));
  NoiseSensSolveArgs& sa = N.sa; std::memset(&sa, 0, sizeof(sa));
  sa.bmeta = N.pa.bmeta; sa.G = c->ac.d_dumpG.p; sa.C = c->ac.d_dumpC.p; sa.R = B.d_R.p; sa.omega = c->ac.d_omega.p; sa.skip = c->sens.d_skip.p;
  sa.ds = ds; sa.S = S; sa.n_freq = n_freq; sa.n_par = 0; sa.comp = N.comp; sa.row_out = N.pa.row_out; sa.n_tab = N.n_tab;
  sa.na = c->ac.d_noise_a.p; sa.nb = c->ac.d_noise_b.p; sa.pwr = c->ac.d_noise_pwr.p; sa.ex = c->ac.d_noise_exp.p; sa.dpwr = B.d_dpwr.p;
  sa.y_out = B.d_y.p; sa.dpsd_out = B.d_dpsd.p; sa.fail = c->sens.d_fail.p;
  NoiseSensRhsArgs& ra = N.ra; std::memset(&ra, 0, sizeof(ra));
  ra.bmeta = N.pa.bmeta; ra.skip = c->sens.d_skip.p; ra.y = B.d_y.p; ra.omega = c->ac.d_omega.p; ra.ds = ds; ra.S = S; ra.n_freq = n_freq; ra.comp = N.comp;
  return launch_noisesens(c, sa, n_freq, S, N.ncb, 0, &N.y_ms, &N.n_ysolve);
}

// one difference of dumps into R_k, one difference of tables into dpwr_k (the `accumulate` of acsens_explicit_term / acsens_state_term)
static int noisesens_accumulate(ch_circuit* c, NoiseSensRun& N, int k, bool minus_is_op, const double* den_k) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t stream = c->ctx->stream;
  NoiseSensitivity& B = c->nsens;
  const int S = N.S, n_freq = N.ra.n_freq;
  NoiseSensRhsArgs b = N.ra;
  b.Gp = c->sens.d_Gp.p; b.Cp = c->sens.d_Cp.p; b.Gm = minus_is_op ? c->ac.d_dumpG.p : c->sens.d_Gm.p; b.Cm = minus_is_op ? c->ac.d_dumpC.p : c->sens.d_Cm.p;
  b.den = den_k; b.R = B.d_R.p + (size_t)k * N.r_stride;
  hipLaunchKernelGGL(noisesens_rhs_kernel, dim3(S, (n_freq + ACSENS_FT - 1) / ACSENS_FT, (N.ncb + 63) / 64), dim3(64), 0, stream, b);
  HIPCHK(hipGetLastError());
  NoiseSensDpwrArgs d; std::memset(&d, 0, sizeof(d));
  d.pwr_p = B.d_pwr_p.p; d.ex_p = B.d_ex_p.p; d.pwr_m = minus_is_op ? c->ac.d_noise_pwr.p : B.d_pwr_m.p; d.ex_m = minus_is_op ? c->ac.d_noise_exp.p : B.d_ex_m.p;
  d.ex0 = c->ac.d_noise_exp.p; d.den = den_k; d.skip = c->sens.d_skip.p; d.dpwr = B.d_dpwr.p + (size_t)k * N.nT; d.ex_moved = B.d_ex_moved.p + k; d.S = S; d.n_tab = N.n_tab;
  if (N.nT > 0) hipLaunchKernelGGL(noisesens_dpwr_kernel, dim3((unsigned)((N.nT + 255) / 256)), dim3(256), 0, stream, d);
  HIPCHK(hipGetLastError());
  N.n_small += 2;
  return CH_OK;
}
// the source table with the tables of `a` and the sources `src` at the state X, into the scratch of `sign`
static int noisesens_build_table(ch_circuit* c, NoiseSensRun& N, const NewtonArgs& a, SourceTables src, const double* X, int sign, const double* npar) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  NoiseSensitivity& B = c->nsens;
  c->eval_sources(0.0, N.mode, N.sv_h, N.kv_h, src);
  HIPCHK(B.d_kv.upload(N.kv_h, c->ctx->stream));
  NoiseTabArgs t = N.tab0;
  t.dcls_local = a.dcls_local; t.dpar = a.dpar; t.dmult = a.dmult; t.vapar = a.vapar; t.temp_s = a.temp_s; t.gmin_s = a.gmin_s; t.X = X; t.kv = B.d_kv.p;
  t.na = B.d_na.p; t.nb = B.d_nb.p; t.pwr = sign > 0 ? B.d_pwr_p.p : B.d_pwr_m.p; t.ex = sign > 0 ? B.d_ex_p.p : B.d_ex_m.p;
  N.n_small += 1 + N.mos_noise;
  return noise_table_launch(c, t, N.mos_noise, a.dcls, a.mosp, npar);
}

// 4. explicit term: every perturbed evaluation leaves G+-, C+- and, through the table kernels with the perturbed tables, pwr+-
static int noisesens_explicit_term(ch_circuit* c, int32_t n_par, const int32_t* slot_ids, NoiseSensRun& N) {
  const Analysis& A = c->desc.A;
  const std::vector<double>& npar_own = c->ac.mos_npar_host;   // what launch_mos_noise built and uploaded for the operating point's table
  auto accumulate = [&](int k, bool minus_is_op, const double* den_k) { return noisesens_accumulate(c, N, k, minus_is_op, den_k); };
  return sens_perturbed_evals(c, n_par, slot_ids, true, [&](int k, bool central) { return acsens_explicit_term(c, N, k, central, accumulate); }, N,
                              [&](int k, int sign, const NewtonArgs& a, SourceTables src) {
    const double* npar = c->ac.d_mos_npar.p;
    if (N.mos_noise && a.n_mos_cls == c->tab.n_cls + 1) {   // the slot is an instance parameter of a MOSFET, which runs on class n_cls: one more row for it
      const int hd = c->desc.slot_a[slot_ids[k]];
      const int m = (int)(std::find(A.mos_hdev.begin(), A.mos_hdev.end(), hd) - A.mos_hdev.begin());
      const std::vector<double> ext = noisesens_npar_extra_row(npar_own, c->tab.n_cls, CH_B4N_NPAR, m < (int)A.mos_hdev.size() ? c->tab.mos_cls[m] : -1);
      if (ext.empty()) { c->set_err("ch_noise_sens: no MOSFET class behind the perturbed instance"); return (int)CH_ERR_INTERNAL; }
      if (c->nsens.d_npar.upload(ext, c->ctx->stream) != hipSuccess) return (int)CH_ERR_DEVICE;
      npar = c->nsens.d_npar.p;
    }
    return noisesens_build_table(c, N, a, src, c->nwt.d_X.p, sign, npar);
  });
}

// 7. PSD and dS/dp back (a sample whose operating point failed is not served), the statistics and the return code
static int noisesens_finish(ch_circuit* c, int32_t n_par, const int32_t* slot_ids, int32_t n_freq, double* psd_out, double* dpsd_out, NoiseSensRun& N, ch_stats* stats) {
  const int S = N.S;
  const size_t nd = (size_t)S * n_freq * n_par;
  std::vector<int> ex_moved(n_par, 0);
  int fail = 0, mfail = 0;   // a singular Y; the flag of the MOSFET table kernel
  bool okc = hipMemcpy(psd_out, c->ac.d_psd.p, (size_t)S * n_freq * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(dpsd_out, c->nsens.d_dpsd.p, nd * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(ex_moved.data(), c->nsens.d_ex_moved.p, n_par * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess &&
             hipMemcpy(&fail, c->sens.d_fail.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  if (okc && N.mos_noise) okc = hipMemcpy(&mfail, c->ac.d_mos_fail.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  if (!okc) { c->set_err("noise sensitivities: reading the result back failed"); return CH_ERR_DEVICE; }
  for (int s = 0; s < S; ++s) {
    if (N.skip[s]) {   // not served: the operating point failed
      std::fill(psd_out + (size_t)s * n_freq, psd_out + (size_t)(s + 1) * n_freq, CH_NAN);
      std::fill(dpsd_out + (size_t)s * n_freq * n_par, dpsd_out + (size_t)(s + 1) * n_freq * n_par, CH_NAN);
    } else for (int f = 0; f < n_freq; ++f) if (std::isnan(psd_out[(size_t)s * n_freq + f])) fail = 1;   // (ac_block_kernel's own flag also counts the samples not served)
  }
  const int nblk = N.nblk;
  ch_stats& st = N.st;
  c->stats.fill(st);
  st.device_seconds += (N.solve_ms + N.y_ms + N.psolve_ms) * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + N.n_solve_launches + N.n_ysolve + N.n_csolve + N.n_small + 2 * N.n_state + 2 + N.mos_noise;
  st.nf += (int64_t)(N.n_eval + 1) * S; st.njacs += (int64_t)(N.n_eval + 1) * S;
  st.nfactors += (int64_t)nblk * N.n_chunks + (int64_t)3 * S * n_freq; st.nsolve += (int64_t)nblk * n_par + (int64_t)S * n_freq * (n_par + 3);
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - N.t0).count();
  if (stats) *stats = st;
  if (c->host_profile)
    std::fprintf(stderr, "[noisesens] operating point %.3f ms, explicit evaluations %.3f ms, state evaluations (%d parameters) %.3f ms (host wall, table, rhs and dpwr launches included), "
                 "%d small launches, real solve %.3f ms, y solve %.3f ms, parameter solve %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3,
                 std::chrono::duration<double>(N.t_eval1 - N.t_eval0).count() * 1e3, N.n_state, std::chrono::duration<double>(N.t_state1 - N.t_state0).count() * 1e3,
                 N.n_small, (double)N.solve_ms, (double)N.y_ms, (double)N.psolve_ms, st.wall_seconds * 1e3);
  if (mfail) { c->set_err("MOSFET noise: a BSIM4 card without an intrinsic charge model (capmod 0 or xpart < 0) has no inversion charge to take the channel noise from"); return CH_ERR_UNSUPPORTED; }
  for (int k = 0; k < n_par; ++k) if (ex_moved[k]) {
    c->set_err("ch_noise_sens: slot " + std::to_string(slot_ids[k]) + " moves the exponent of a flicker source, which is not differentiated");
    return CH_ERR_UNSUPPORTED;
  }
  return sens_outcome(c, "noise sensitivities", N, fail);
}

static int ch_noise_sens_impl(ch_circuit* c, const ch_dc_opts* o, const ch_noise_opts* no, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t out_kind,
                              int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out, double* dpsd_out, double* dc_sens_out, int32_t* status_out,
                              ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  NoiseSensRun N;
  int rc = noisesens_check(c, no, n_par, slot_ids, so, out_kind, out_index, n_freq, freqs_hz, psd_out, dpsd_out, N);
  if (rc != CH_OK) return rc;
  rc = sens_operating_point(c, o, "noise sensitivities", n_par, nullptr, status_out, N);
  if (rc != CH_OK) return rc;
  if (N.u_out < 0) return noisesens_held_output(c, n_par, slot_ids, n_freq, psd_out, dpsd_out, dc_sens_out, N, stats);
  rc = noisesens_table_and_y(c, n_par, n_freq, freqs_hz, N);
  if (rc != CH_OK) return rc;
  rc = noisesens_explicit_term(c, n_par, slot_ids, N);
  if (rc != CH_OK) return rc;
  rc = sens_real_solves(c, n_par, N, dc_sens_out);   // s_k = dx*/dp_k (what ch_dc_sens returns)
  if (rc != CH_OK) return rc;
  const double* Xs = c->nwt.d_X.p + (size_t)ACSENS_X_SLOT * c->nwt.base.slot_stride;   // 5. state term: the source table is rebuilt at the shifted state
  rc = acsens_state_term(c, n_par, N, [&](int sign) { return noisesens_build_table(c, N, c->nwt.base, c->own_sources(), Xs, sign, c->ac.d_mos_npar.p); },
                         [&](int k, bool minus_is_op, const double* den_k) { return noisesens_accumulate(c, N, k, minus_is_op, den_k); });
  if (rc != CH_OK) return rc;
  N.sa.n_par = n_par;   // 6. the transposed solves with every parameter, and the reduction over the table
  rc = launch_noisesens(c, N.sa, n_freq, N.S, N.ncb, n_par, &N.psolve_ms, &N.n_csolve);
  if (rc != CH_OK) return rc;
  return noisesens_finish(c, n_par, slot_ids, n_freq, psd_out, dpsd_out, N, stats);
}
}  // extern "C++"
