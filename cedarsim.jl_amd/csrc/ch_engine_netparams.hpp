// ch_engine_netparams.hpp — N-port network analysis: the S, Y and Z parameters of a circuit seen from P voltage-source ports, with
// their parameter sensitivities and frequency-domain measures (ch_net_params).  With Y = G + jwC at the operating point,
//   Y x_k = b_k (port k at 1 V, the others AC shorts),   Yp[j][k] = -x_k[row_i(j)],   Y^T l_j = e_row_i(j),
//   dYp[j][k]/dp = l_j^T (dY/dp) x_k,   S = (I - y)(I + y)^-1 with y = sqrt(z0) Yp sqrt(z0),   Z = Yp^-1,
//   dS = -1/2 (I + S)(sqrt(z0) dYp sqrt(z0))(I + S),   dZ = -Z dYp Z:
// 2P substitutions per frequency and P^2 bilinear forms per parameter, no per-parameter solve.  The sequence is
// ch_loop_gain's: dY/dp is the matrix ch_ac_sens forms (ch_engine_sens.hpp's front half, passes, chunk launcher and outcome rule),
// the linearisation and the right-hand side are ch_engine_ac.hpp's, the measure launch ch_engine_fmeasure.hpp's; the HIP-free half is
// ch_netparams_host.hpp, the kernels are in ch_netparams_kernels.hpp.  Included by ch_engine.hip behind ch_engine_loopgain.hpp.
#pragma once

extern "C++" {

// Y(w) (and, with a.adjoint, Y^T(w)) solves of the ports' block, one system per (frequency, sample).  Up to 96 unknowns one wavefront
// with factors and panel in LDS; above that the 256-thread variant on a global workspace, a chunk of frequencies per launch.
static int launch_netparams(ch_circuit* c, NetParamsSolveArgs& a, int n_freq, int S, int nc, float* ms_out, int* n_launches) {
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  hipStream_t st = c->ctx->stream;
  const bool in_lds = nc <= 96;
  if (in_lds) {
    size_t budget = 0;
    HIPCHK(lds_budget_doubles((const void*)netparams_solve_kernel<64>, &budget));
    if (netparams_lds_doubles(nc, a.P) > budget) { c->set_err("ch_net_params: the factors of the ports' block do not fit the LDS"); return CH_ERR_INTERNAL; }
  }
  const size_t per = in_lds ? 0 : netparams_work_doubles(nc, a.P);
  a.work_per = (long)per;
  return launch_freq_chunks(c, "ch_net_params", n_freq, S, per, [&](int f0, int nf, double* work) {
    a.f0 = f0; a.work = work;
    if (in_lds) hipLaunchKernelGGL(netparams_solve_kernel<64>, dim3(nf, S), dim3(64), netparams_lds_doubles(nc, a.P) * sizeof(double), st, a);
    else hipLaunchKernelGGL(netparams_solve_kernel<256>, dim3(nf, S), dim3(256), 0, st, a);
  }, ms_out, n_launches);
}

static int ch_net_params_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_ports, const int32_t* port_devs, const double* z0, int32_t n_par, const int32_t* slot_ids,
                              const ch_sens_opts* so, int32_t n_freq, const double* freqs_hz, double* S_out, double* Y_out, double* Z_out, double* dS_out, double* dY_out,
                              double* dZ_out, int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status,
                              int32_t* sample_status, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  if (stats) std::memset(stats, 0, sizeof(*stats));   // a call refused in front of the DC solve has run nothing
  std::string who = "ch_net_params";
  auto set_err = [&](const std::string& m) { c->set_err(who + ": " + m); };
  auto bad = [&](const std::string& m) { set_err(m); return (int)CH_ERR_INVALID; };
  auto port_name = [&](int j) { return "port " + std::to_string(j + 1) + " (device " + std::to_string(port_devs[j]) + ")"; };
  // ---- refusals, all before the DC solve ----
  if (n_ports < 1 || n_ports > CH_NET_MAX_PORTS || !port_devs || !z0) return bad("between 1 and " + std::to_string(CH_NET_MAX_PORTS) + " ports, each with its reference impedance");
  const int P = n_ports, PP = P * P;
  for (int j = 0; j < P; ++j) if (!(z0[j] > 0.0 && z0[j] < HUGE_VAL)) return bad(port_name(j) + ": its reference impedance must be real, finite and positive");
  if (n_meas < 0 || (n_meas > 0 && (!specs || !out_value || !out_status))) return bad("measures without their specs and output arrays");
  if (!S_out && !Y_out && !Z_out && n_meas == 0) return bad("nothing asked for: S_out, Y_out, Z_out or at least one measure");
  if (n_par < 0 || (n_par == 0 && (dS_out || dY_out || dZ_out || out_sens))) return bad("sensitivities asked for without parameters");
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
  if (n_meas > 0) { std::string why; if (!fmeasure_check(n_freq, freqs_hz, 3 * PP, n_meas, specs, why)) return bad(why); }   // rows: kind * P^2 + j * P + k
  rc = smallsignal_prepare(c, who, "dense complex LU");
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  std::vector<int> u_ip; int bad_port = 0;
  if (const char* w = netparams_port_check(c->desc.dev, c->desc.src, A, P, port_devs, u_ip, bad_port)) return bad(bad_port > 0 ? port_name(bad_port - 1) + ": " + w : std::string(w));
  for (int k = 0; k < n_par; ++k) if (netparams_slot_moves_b(c->desc.slot_kind, c->desc.slot_a, slot_ids[k], P, port_devs)) {
    for (int j = 0; j < P; ++j) if (c->desc.slot_a[slot_ids[k]] == port_devs[j]) set_err(port_name(j) + ": a port's own multiplier is not a supported slot (it moves the right-hand sides)");
    return CH_ERR_UNSUPPORTED;
  }
  int comps[CH_NET_MAX_PORTS], rows[CH_NET_MAX_PORTS];
  for (int j = 0; j < P; ++j) comps[j] = c->ac_comp_of(u_ip[j]);
  if (const int j = netparams_split_port(comps, P); j >= 0) {
    set_err(port_name(j) + ": its branch current lies in another block than port 1's (ports in separate blocks are not supported)"); return CH_ERR_UNSUPPORTED;
  }
  const int comp = comps[0], ncb = c->ac_nc(comp);
  for (int j = 0; j < P; ++j) {
    rows[j] = u_ip[j] - c->ac_uofs(comp);
    if (rows[j] < 0 || rows[j] >= ncb) { set_err("internal: " + port_name(j) + " lies outside its block"); return CH_ERR_INTERNAL; }
  }
  // a kind's rows exist on the device only if an output or a measure names it; Yp always exists
  bool want[3] = {S_out || dS_out, true, Z_out || dZ_out};
  for (int m = 0; m < n_meas; ++m) {
    const ch_fmeasure_side* sides[2] = {&specs[m].s1, fmeas_uses_s2(specs[m].kind) ? &specs[m].s2 : nullptr};
    for (const ch_fmeasure_side* sd : sides) if (sd) { want[sd->row_a / PP] = true; if (sd->row_b >= 0) want[sd->row_b / PP] = true; }
  }
  int slot_of[3], n_kinds = 0;
  slot_of[CH_NET_Y] = n_kinds++;
  slot_of[CH_NET_S] = want[CH_NET_S] ? n_kinds++ : -1;
  slot_of[CH_NET_Z] = want[CH_NET_Z] ? n_kinds++ : -1;
  // ---- operating point (a sample that fails keeps its status, the others are served), G, C, b ----
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
  // ---- one workspace: values [kind][P^2] rows | x_k, l_j | derivative rows [kind][P^2][n_par] | conversion work | sqrt(z0) | port rows |
  //      axes | specs | values | status | sens ----
  const long nf = n_freq;
  const size_t n_fs = (size_t)nf * S, n_out = (size_t)n_meas * S, row = 2 * n_fs, n_val = (size_t)PP * row, n_der = n_val * (size_t)n_par;
  const size_t o_V = 0, o_vec = o_V + n_kinds * n_val, o_dV = o_vec + (n_par > 0 ? (size_t)2 * P * n_fs * ncb * 2 : 0), o_w = o_dV + n_kinds * n_der,
               o_rz = o_w + (n_kinds > 1 ? n_val : 0), o_rows = o_rz + P, o_ax = o_rows + (P + 1) / 2, o_sp = o_ax + 2 * (size_t)nf,
               o_val = o_sp + (sizeof(ch_fmeasure_spec) * (size_t)n_meas + 7) / 8, o_st = o_val + n_out, o_sens = o_st + (n_out + 1) / 2,
               total = o_sens + n_out * (size_t)n_par;
  ScopedWorkspace work;
  if (work.alloc(std::max<size_t>(1, total)) != hipSuccess) { set_err("out of device memory for the rows"); return CH_ERR_DEVICE; }
  auto val_of = [&](int kind) { return slot_of[kind] < 0 ? (double*)nullptr : work.p + o_V + slot_of[kind] * n_val; };
  auto der_of = [&](int kind) { return slot_of[kind] < 0 || n_par == 0 ? (double*)nullptr : work.p + o_dV + slot_of[kind] * n_der; };
  double rz[CH_NET_MAX_PORTS];
  for (int j = 0; j < P; ++j) rz[j] = std::sqrt(z0[j]);
  HIPCHK(hipMemcpyAsync(work.p + o_rz, rz, P * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(work.p + o_rows, rows, P * sizeof(int), hipMemcpyHostToDevice, stream));
  // ---- the solves ----
  NetParamsSolveArgs sa; std::memset(&sa, 0, sizeof(sa));
  sa.bmeta = bmeta; sa.G = c->ac.d_dumpG.p; sa.C = c->ac.d_dumpC.p; sa.b = c->ac.d_dumpF.p; sa.omega = c->ac.d_omega.p; sa.skip = c->sens.d_skip.p;
  sa.rows = (const int*)(work.p + o_rows); sa.ds = ds; sa.S = S; sa.n_freq = n_freq; sa.comp = comp; sa.P = P; sa.adjoint = n_par > 0 ? 1 : 0;
  sa.Yp = val_of(CH_NET_Y); sa.vec = work.p + o_vec; sa.fail = c->ac.d_acfail.p;
  float csolve_ms = 0.0f; int n_csolve = 0, n_small = 0;
  rc = launch_netparams(c, sa, n_freq, S, ncb, &csolve_ms, &n_csolve);
  if (rc != CH_OK) return rc;
  // ---- dYp/dp: the two terms of dY/dp_k, each difference folded into dYp_k by P^2 bilinear forms ----
  if (n_par > 0) {
    rc = acsens_alloc_differences(c, n_par, R);
    if (rc != CH_OK) return rc;
    HIPCHK(hipMemsetAsync(der_of(CH_NET_Y), 0, n_der * sizeof(double), stream));
    NetParamsBilinearArgs ba; std::memset(&ba, 0, sizeof(ba));
    ba.bmeta = bmeta; ba.skip = c->sens.d_skip.p; ba.vec = work.p + o_vec; ba.omega = c->ac.d_omega.p; ba.ds = ds; ba.S = S; ba.n_freq = n_freq; ba.comp = comp; ba.P = P;
    ba.row_ld = (long)n_par * (long)n_fs;
    auto accumulate = [&](int k, bool minus_is_op, const double* den_k) {
      NetParamsBilinearArgs b = ba;
      b.Gp = c->sens.d_Gp.p; b.Cp = c->sens.d_Cp.p; b.Gm = minus_is_op ? c->ac.d_dumpG.p : c->sens.d_Gm.p; b.Cm = minus_is_op ? c->ac.d_dumpC.p : c->sens.d_Cm.p;
      b.den = den_k; b.dY = der_of(CH_NET_Y) + (size_t)k * row;
      hipLaunchKernelGGL(netparams_bilinear_kernel, dim3(S, (n_freq + NET_FT - 1) / NET_FT, P), dim3(256), 0, stream, b);
      ++n_small;
      return hipGetLastError() == hipSuccess ? (int)CH_OK : (int)CH_ERR_DEVICE;
    };
    rc = sens_perturbed_evals(c, n_par, slot_ids, true, [&](int k, bool central) { return acsens_explicit_term(c, R, k, central, accumulate); }, R);
    if (rc != CH_OK) return rc;
    rc = sens_real_solves(c, n_par, R, nullptr);   // s_k = dx*/dp_k (what ch_dc_sens returns)
    if (rc != CH_OK) return rc;
    rc = acsens_state_term(c, n_par, R, [](int) { return (int)CH_OK; }, accumulate);
    if (rc != CH_OK) return rc;
  }
  // ---- Yp, dYp -> the S and Z rows; skipped when nobody asked for either ----
  if (n_kinds > 1) {
    NetParamsConvertArgs ca; std::memset(&ca, 0, sizeof(ca));
    ca.Yp = val_of(CH_NET_Y); ca.dYp = der_of(CH_NET_Y); ca.Sm = val_of(CH_NET_S); ca.dSm = der_of(CH_NET_S); ca.Zm = val_of(CH_NET_Z); ca.dZm = der_of(CH_NET_Z);
    ca.work = work.p + o_w; ca.rz = work.p + o_rz; ca.skip = c->sens.d_skip.p; ca.n_fs = (long)n_fs; ca.S = S; ca.P = P; ca.n_par = n_par;
    hipLaunchKernelGGL(netparams_convert_kernel, dim3((unsigned)((n_fs + 63) / 64)), dim3(64), 0, stream, ca);
    HIPCHK(hipGetLastError());
    ++n_small;
  }
  // ---- the measures, on the rows where they lie: the kinds that exist, compact ----
  if (n_meas > 0) {
    std::vector<ch_fmeasure_spec> sp(specs, specs + n_meas);
    auto move = [&](int32_t& r) { if (r >= 0) r = slot_of[r / PP] * PP + r % PP; };
    for (ch_fmeasure_spec& m : sp) {
      move(m.s1.row_a); move(m.s1.row_b);
      if (fmeas_uses_s2(m.kind)) { move(m.s2.row_a); move(m.s2.row_b); } else { m.s2 = m.s1; }
    }
    std::vector<double> ax;
    fmeasure_axes(n_freq, freqs_hz, sp, ax);
    HIPCHK(hipMemcpyAsync(work.p + o_ax, ax.data(), ax.size() * sizeof(double), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(work.p + o_sp, sp.data(), sizeof(ch_fmeasure_spec) * (size_t)n_meas, hipMemcpyHostToDevice, stream));
    FMeasureArgs a; std::memset(&a, 0, sizeof(a));
    a.rows.f = work.p + o_ax; a.rows.ulog = work.p + o_ax + nf; a.rows.nf = nf; a.rows.n_par = n_par;
    a.rows.H = work.p + o_V; a.rows.ldH = S; a.rows.dH = n_par > 0 ? work.p + o_dV : nullptr; a.rows.ldS = S;
    a.specs = (const ch_fmeasure_spec*)(work.p + o_sp); a.n_meas = n_meas; a.n_samples = S;
    a.value = work.p + o_val; a.status = (int*)(work.p + o_st); a.sens = n_par > 0 ? work.p + o_sens : nullptr; a.ldo = S; a.skip = c->sens.d_skip.p;
    fmeasure_launch(stream, measure_lanes_form(S), a);
    HIPCHK(hipGetLastError());
    ++n_small;
    HIPCHK(hipMemcpyAsync(out_value, work.p + o_val, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(out_status, work.p + o_st, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (n_par > 0 && out_sens) HIPCHK(hipMemcpyAsync(out_sens, work.p + o_sens, n_out * (size_t)n_par * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  // ---- back: only what was asked for, [P^2][n_freq][S] -> [S][n_freq][P^2] (and [P^2][n_par][n_freq][S] -> [S][n_freq][n_par][P^2]) on the host ----
  double* outs[3] = {S_out, Y_out, Z_out}; double* douts[3] = {dS_out, dY_out, dZ_out};
  std::vector<double> hV[3], hdV[3];
  int fail = 0;
  for (int kd = 0; kd < 3; ++kd) {
    if (outs[kd]) { hV[kd].resize(n_val); HIPCHK(hipMemcpyAsync(hV[kd].data(), val_of(kd), n_val * sizeof(double), hipMemcpyDeviceToHost, stream)); }
    if (douts[kd]) { hdV[kd].resize(n_der); HIPCHK(hipMemcpyAsync(hdV[kd].data(), der_of(kd), n_der * sizeof(double), hipMemcpyDeviceToHost, stream)); }
  }
  HIPCHK(hipMemcpyAsync(&fail, c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int kd = 0; kd < 3; ++kd) for (int s = 0; s < S; ++s) for (long f = 0; f < nf; ++f) for (int e = 0; e < PP; ++e) for (int q = 0; q < 2; ++q) {
    const size_t fs = (size_t)f * S + s, sf = (size_t)s * nf + f;
    if (outs[kd]) outs[kd][(sf * PP + e) * 2 + q] = R.skip[s] ? CH_NAN : hV[kd][((size_t)e * n_fs + fs) * 2 + q];
    if (douts[kd]) for (int k = 0; k < n_par; ++k)
      douts[kd][((sf * n_par + k) * PP + e) * 2 + q] = R.skip[s] ? CH_NAN : hdV[kd][(((size_t)e * n_par + k) * n_fs + fs) * 2 + q];
  }
  // ---- statistics and the return code ----
  ch_stats& st = R.st;
  if (n_par == 0) {
    st.nsolve += (int64_t)(P - 1) * S * n_freq;   // (ac_finish counts one substitution per system)
    rc = ac_finish(c, "network analysis", st, R.t0, n_freq, 2 + n_csolve + n_small, fail, stats);
    return rc != CH_OK ? rc : sens_outcome(c, "network analysis", R, 0);
  }
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - R.t0).count();
  c->stats.fill(st);
  st.device_seconds += (R.solve_ms + csolve_ms) * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + R.n_solve_launches + n_csolve + n_small + 2 * R.n_state + 2;
  st.nf += (int64_t)(R.n_eval + 2) * S; st.njacs += (int64_t)(R.n_eval + 1) * S;
  st.nfactors += (int64_t)R.nblk * R.n_chunks + (int64_t)2 * S * n_freq; st.nsolve += (int64_t)R.nblk * n_par + (int64_t)2 * P * S * n_freq;
  if (c->host_profile)
    std::fprintf(stderr, "[netparams] operating point %.3f ms, explicit evaluations %.3f ms, state evaluations (%d parameters) %.3f ms (host wall, bilinear launches included), "
                 "%d small launches, real solve %.3f ms, complex solve %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3,
                 std::chrono::duration<double>(R.t_eval1 - R.t_eval0).count() * 1e3, R.n_state, std::chrono::duration<double>(R.t_state1 - R.t_state0).count() * 1e3,
                 n_small, (double)R.solve_ms, (double)csolve_ms, st.wall_seconds * 1e3);
  if (stats) *stats = st;
  return sens_outcome(c, "network analysis", R, fail);
}
}  // extern "C++"
