// ch_engine_loopgain.hpp — loop-gain (stability) analysis of a closed loop at a voltage-source probe, with its parameter sensitivities
// and frequency-domain measures (ch_loop_gain).  The probe x -> y sits in the loop wire; with Y = G + jwC at the operating point,
//   Y x_v = b_v (the probe at 1 V: ac_rhs's vector),   Y x_i = b_i (unit current into x),   u = x_v[x] - x_i[i_p],   T = u / (1 - u),
// and, with Y^T l_x = e_x, Y^T l_i = e_ip,   du/dp_k = -l_x^T (dY/dp_k) x_v + l_i^T (dY/dp_k) x_i,   dT/dp_k = (du/dp_k) / (1 - u)^2:
// four substitutions per frequency and two bilinear forms per parameter, no per-parameter solve.  dY/dp_k is the
// matrix ch_ac_sens forms: the front half — operating point, perturbed evaluations, real solves — the two passes over the parameters
// (acsens_explicit_term, acsens_state_term), the chunk launcher and the outcome rule are ch_engine_sens.hpp's, the linearisation and
// b_v ch_engine_ac.hpp's, the measure launch ch_engine_fmeasure.hpp's; the HIP-free half is ch_loopgain_host.hpp, the kernels are in
// ch_loopgain_kernels.hpp.  Included by ch_engine.hip behind ch_engine_fmeasure.hpp.
#pragma once

extern "C++" {

// Y(w) (and, with a.adjoint, Y^T(w)) solves of the probe's block, one system per (frequency, sample).  Up to 96 unknowns one wavefront
// with factors and panel in LDS; above that the 256-thread variant on a global workspace, a chunk of frequencies per launch.
static int launch_loopgain(ch_circuit* c, LoopGainSolveArgs& a, int n_freq, int S, int nc, float* ms_out, int* n_launches) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  const bool in_lds = nc <= 96;
  if (in_lds) {
    size_t budget = 0;
    HIPCHK(lds_budget_doubles((const void*)loopgain_solve_kernel<64>, &budget));
    if (loopgain_lds_doubles(nc) > budget) { c->set_err("ch_loop_gain: the factors of the probe's block do not fit the LDS"); return CH_ERR_INTERNAL; }
  }
  const size_t per = in_lds ? 0 : loopgain_work_doubles(nc);
  a.work_per = (long)per;
  return launch_freq_chunks(c, "ch_loop_gain", n_freq, S, per, [&](int f0, int nf, double* work) {
    a.f0 = f0; a.work = work;
    if (in_lds) hipLaunchKernelGGL(loopgain_solve_kernel<64>, dim3(nf, S), dim3(64), loopgain_lds_doubles(nc) * sizeof(double), st, a);
    else hipLaunchKernelGGL(loopgain_solve_kernel<256>, dim3(nf, S), dim3(256), 0, st, a);
  }, ms_out, n_launches);
}

static int ch_loop_gain_impl(ch_circuit* c, const ch_dc_opts* o, int32_t probe_dev, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq,
                             const double* freqs_hz, double* T_out, double* dT_out, int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value, double* out_sens,
                             int32_t* out_status, int32_t* sample_status, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  if (stats) std::memset(stats, 0, sizeof(*stats));   // a call refused in front of the DC solve has run nothing
  const std::string who = "ch_loop_gain (probe: device " + std::to_string(probe_dev) + ")";
  auto set_err = [&](const std::string& m) { c->set_err(who + ": " + m); };
  auto bad = [&](const std::string& m) { set_err(m); return (int)CH_ERR_INVALID; };
  // ---- refusals, all before the DC solve ----
  if (n_meas < 0 || (n_meas > 0 && (!specs || !out_value || !out_status))) return bad("measures without their specs and output arrays");
  if (!T_out && n_meas == 0) return bad("nothing asked for: T_out or at least one measure");
  if (n_par < 0 || (n_par == 0 && (dT_out || out_sens))) return bad("sensitivities asked for without parameters");
  if (n_freq < 1 || !freqs_hz) return bad("at least one frequency");
  SensRun R;
  // from the DC solve on, whatever way the call ends, its statistics go out: a refusal behind the operating point would show its work
  struct PublishStats { ch_stats* out = nullptr; const ch_stats* st = nullptr; ~PublishStats() { if (out) *out = *st; } } publish;
  publish.st = &R.st;
  ch_sens_opts_default(&R.opt);
  int rc = CH_OK;
  if (n_par > 0) {
    rc = sens_check_args(c, who.c_str(), n_par, slot_ids, nullptr, so, R.opt, false);
    if (rc != CH_OK) return rc;
  }
  if (check_frequencies(c, n_freq, freqs_hz) != CH_OK) return bad("frequencies must be finite and non-negative");
  if (n_meas > 0) { std::string why; if (!fmeasure_check(n_freq, freqs_hz, 1, n_meas, specs, why)) return bad(why); }   // rows: 0 = T
  rc = smallsignal_prepare(c, who, "dense complex LU");
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  LoopGainProbe P;
  if (const char* w = loopgain_probe_check(c->desc.dev, c->desc.src, A, probe_dev, P)) return bad(w);
  for (int k = 0; k < n_par; ++k) if (loopgain_slot_moves_b(c->desc.slot_kind, c->desc.slot_a, slot_ids[k], probe_dev)) {
    set_err("the probe's own multiplier is not a supported slot (it moves the right-hand sides)"); return CH_ERR_UNSUPPORTED;
  }
  const int comp = c->ac_comp_of(P.u_x), ncb = c->ac_nc(comp), row_x = P.u_x - c->ac_uofs(comp), row_i = P.u_ip - c->ac_uofs(comp);
  if (row_x < 0 || row_x >= ncb || row_i < 0 || row_i >= ncb) { set_err("internal: the probe's node and branch current lie in different blocks"); return CH_ERR_INTERNAL; }
  // ---- operating point (a sample that fails keeps its status, the others are served), G, C, b_v ----
  publish.out = stats;
  rc = sens_operating_point(c, o, who.c_str(), n_par, nullptr, sample_status, R);
  if (rc != CH_OK) return rc;
  const int S = R.S, ds = R.ds;
  hipStream_t stream = c->ctx->stream;
  rc = ac_rhs(c, R.mode);
  if (rc != CH_OK) return rc;
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  const BlockMeta* bmeta = c->ac_bmeta();
  if (!bmeta) return CH_ERR_DEVICE;
  HIPCHK(c->sens.d_skip.upload(R.skip, stream));
  // ---- one workspace: T | u | x_v, x_i, l_x, l_i | du | dT | axes | specs | values | status | sens ----
  const long nf = n_freq;
  const size_t n_fs = (size_t)nf * S, n_out = (size_t)n_meas * S;
  const size_t o_T = 0, o_u = o_T + 2 * n_fs, o_vec = o_u + 2 * n_fs, o_du = o_vec + (n_par > 0 ? (size_t)4 * n_fs * ncb * 2 : 0), o_dT = o_du + 2 * n_fs * n_par,
               o_ax = o_dT + 2 * n_fs * n_par, o_sp = o_ax + 2 * (size_t)nf, o_val = o_sp + (sizeof(ch_fmeasure_spec) * (size_t)n_meas + 7) / 8, o_st = o_val + n_out,
               o_sens = o_st + (n_out + 1) / 2, total = o_sens + n_out * (size_t)n_par;
  ScopedWorkspace work;
  if (work.alloc(std::max<size_t>(1, total)) != hipSuccess) { set_err("out of device memory for the rows"); return CH_ERR_DEVICE; }
  // ---- the solves ----
  LoopGainSolveArgs sa; std::memset(&sa, 0, sizeof(sa));
  sa.bmeta = bmeta; sa.G = c->ac.d_dumpG.p; sa.C = c->ac.d_dumpC.p; sa.b = c->ac.d_dumpF.p; sa.omega = c->ac.d_omega.p; sa.skip = c->sens.d_skip.p;
  sa.ds = ds; sa.S = S; sa.n_freq = n_freq; sa.comp = comp; sa.row_x = row_x; sa.row_i = row_i; sa.adjoint = n_par > 0 ? 1 : 0;
  sa.bi = loopgain_bi_entry(LOOPGAIN_BI_TERMINAL);
  sa.T_out = work.p + o_T; sa.u_out = work.p + o_u; sa.vec = work.p + o_vec; sa.fail = c->ac.d_acfail.p;
  float csolve_ms = 0.0f; int n_csolve = 0, n_small = 0;
  rc = launch_loopgain(c, sa, n_freq, S, ncb, &csolve_ms, &n_csolve);
  if (rc != CH_OK) return rc;
  // ---- dT/dp: the two terms of dY/dp_k, each difference folded into du_k by two bilinear forms ----
  if (n_par > 0) {
    rc = acsens_alloc_differences(c, n_par, R);
    if (rc != CH_OK) return rc;
    HIPCHK(hipMemsetAsync(work.p + o_du, 0, 2 * n_fs * n_par * sizeof(double), stream));
    LoopGainBilinearArgs ba; std::memset(&ba, 0, sizeof(ba));
    ba.bmeta = bmeta; ba.skip = c->sens.d_skip.p; ba.vec = work.p + o_vec; ba.omega = c->ac.d_omega.p; ba.ds = ds; ba.S = S; ba.n_freq = n_freq; ba.comp = comp;
    auto accumulate = [&](int k, bool minus_is_op, const double* den_k) {
      LoopGainBilinearArgs b = ba;
      b.Gp = c->sens.d_Gp.p; b.Cp = c->sens.d_Cp.p; b.Gm = minus_is_op ? c->ac.d_dumpG.p : c->sens.d_Gm.p; b.Cm = minus_is_op ? c->ac.d_dumpC.p : c->sens.d_Cm.p;
      b.den = den_k; b.du = work.p + o_du + (size_t)k * 2 * n_fs;
      hipLaunchKernelGGL(loopgain_bilinear_kernel, dim3(S, (n_freq + ACSENS_FT - 1) / ACSENS_FT), dim3(256), 0, stream, b);
      ++n_small;
      return hipGetLastError() == hipSuccess ? (int)CH_OK : (int)CH_ERR_DEVICE;
    };
    rc = sens_perturbed_evals(c, n_par, slot_ids, true, [&](int k, bool central) { return acsens_explicit_term(c, R, k, central, accumulate); }, R);
    if (rc != CH_OK) return rc;
    rc = sens_real_solves(c, n_par, R, nullptr);   // s_k = dx*/dp_k (what ch_dc_sens returns)
    if (rc != CH_OK) return rc;
    rc = acsens_state_term(c, n_par, R, [](int) { return (int)CH_OK; }, accumulate);
    if (rc != CH_OK) return rc;
    const long n_dt = (long)n_fs * n_par;
    hipLaunchKernelGGL(loopgain_dt_kernel, dim3((unsigned)((n_dt + 255) / 256)), dim3(256), 0, stream, (const double*)(work.p + o_u), (const double*)(work.p + o_du), work.p + o_dT,
                       (long)n_fs, (int)n_par);
    HIPCHK(hipGetLastError());
    ++n_small;
  }
  // ---- the measures, on the rows where they lie: row 0 = T ([n_freq][S]), its sensitivity rows dT ([n_par][n_freq][S]) ----
  if (n_meas > 0) {
    std::vector<ch_fmeasure_spec> sp; std::vector<int> used;
    fmeasure_compact(1, n_meas, specs, sp, used);
    std::vector<double> ax;
    fmeasure_axes(n_freq, freqs_hz, sp, ax);
    HIPCHK(hipMemcpyAsync(work.p + o_ax, ax.data(), ax.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(work.p + o_sp, sp.data(), sizeof(ch_fmeasure_spec) * (size_t)n_meas, hipMemcpyHostToDevice, stream));
    FMeasureArgs a; std::memset(&a, 0, sizeof(a));
    a.rows.f = work.p + o_ax; a.rows.ulog = work.p + o_ax + nf; a.rows.nf = nf; a.rows.n_par = n_par;
    a.rows.H = work.p + o_T; a.rows.ldH = S; a.rows.dH = n_par > 0 ? work.p + o_dT : nullptr; a.rows.ldS = S;
    a.specs = (const ch_fmeasure_spec*)(work.p + o_sp); a.n_meas = n_meas; a.n_samples = S;
    a.value = work.p + o_val; a.status = (int*)(work.p + o_st); a.sens = n_par > 0 ? work.p + o_sens : nullptr; a.ldo = S; a.skip = c->sens.d_skip.p;
    fmeasure_launch(stream, measure_lanes_form(S), a);
    HIPCHK(hipGetLastError());
    ++n_small;
    HIPCHK(hipMemcpyAsync(out_value, work.p + o_val, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out_status, work.p + o_st, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (n_par > 0 && out_sens) HIPCHK(hipMemcpyAsync(out_sens, work.p + o_sens, n_out * (size_t)n_par * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  // ---- back: only what was asked for, [n_freq][S] -> [S][n_freq] on the host ----
  std::vector<double> hT(T_out ? 2 * n_fs : 0), hdT(dT_out ? 2 * n_fs * n_par : 0);
  int fail = 0;
  if (T_out) HIPCHK(hipMemcpyAsync(hT.data(), work.p + o_T, hT.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  if (dT_out) HIPCHK(hipMemcpyAsync(hdT.data(), work.p + o_dT, hdT.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&fail, c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int s = 0; s < S; ++s) for (long f = 0; f < nf; ++f) for (int q = 0; q < 2; ++q) {
    const size_t fs = (size_t)f * S + s, sf = (size_t)s * nf + f;
    if (T_out) T_out[2 * sf + q] = R.skip[s] ? CH_NAN : hT[2 * fs + q];
    if (dT_out) for (int k = 0; k < n_par; ++k) dT_out[(sf * n_par + k) * 2 + q] = R.skip[s] ? CH_NAN : hdT[((size_t)k * n_fs + fs) * 2 + q];
  }
  // ---- statistics and the return code ----
  ch_stats& st = R.st;
  if (n_par == 0) {
    rc = ac_finish(c, "loop gain analysis", st, R.t0, n_freq, 2 + n_csolve + n_small, fail, stats);
    return rc != CH_OK ? rc : sens_outcome(c, "loop gain analysis", R, 0);
  }
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - R.t0).count();
  c->stats.fill(st);
  st.device_seconds += (R.solve_ms + csolve_ms) * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + R.n_solve_launches + n_csolve + n_small + 2 * R.n_state + 2;
  st.nf += (int64_t)(R.n_eval + 2) * S; st.njacs += (int64_t)(R.n_eval + 1) * S;
  st.nfactors += (int64_t)R.nblk * R.n_chunks + (int64_t)2 * S * n_freq; st.nsolve += (int64_t)R.nblk * n_par + (int64_t)4 * S * n_freq;
  if (c->host_profile)
    std::fprintf(stderr, "[loopgain] operating point %.3f ms, explicit evaluations %.3f ms, state evaluations (%d parameters) %.3f ms (host wall, bilinear launches included), "
                 "%d small launches, real solve %.3f ms, complex solve %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3,
                 std::chrono::duration<double>(R.t_eval1 - R.t_eval0).count() * 1e3, R.n_state, std::chrono::duration<double>(R.t_state1 - R.t_state0).count() * 1e3,
                 n_small, (double)R.solve_ms, (double)csolve_ms, st.wall_seconds * 1e3);
  if (stats) *stats = st;
  return sens_outcome(c, "loop gain analysis", R, fail);
}
}  // extern "C++"
