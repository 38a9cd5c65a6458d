// ch_engine_fmeasure.hpp — frequency-domain measurements (ch_freq_measure_rows, ch_ac_measure).  Both check the specs and the grid
// (fmeas_spec_check, fmeas_grid_check: before anything is uploaded or solved), map the rows the specs name to a compact set and launch
// one of the two kernels of ch_fmeasure_kernels.hpp: lanes per sample from 64 samples up, the frequency axis split below
// (measure_lanes_form of ch_engine_measure.hpp, the rule of the transient measures).  The form is chosen by the call's sample count, never by a
// chunk's, so a sample's result does not depend on its chunk.  ch_freq_measure_rows uploads host rows, in sample chunks when they
// exceed the cap (CEDARHIP_MEASURE_CAP); ch_ac_measure runs the launches of ch_ac / ch_ac_sens (ac_device_solve, acsens_device_solve),
// gathers the rows out of their device results, copies back values, statuses and sensitivities only and ends with their finish
// (ac_finish, acsens_finish).
// Included by ch_engine.hip behind ch_engine_measure.hpp.
#pragma once

extern "C++" {   // (included inside the extern "C" block of ch_engine.hip)

// the specs with their rows renumbered to the compact set `used` (rows in order of first use); null, or the text of the refusal
static bool fmeasure_check(int32_t n_freq, const double* freqs_hz, int n_rows, int32_t n_meas, const ch_fmeasure_spec* specs, std::string& why) {
  bool any_log = false;
  for (int k = 0; k < n_meas; ++k) {
    if (const char* w = fmeas_spec_check(specs[k], n_rows)) { why = "measure " + std::to_string(k) + ": " + w; return false; }
    any_log = any_log || specs[k].xscale == CH_FX_LOG;
  }
  if (const char* w = fmeas_grid_check(freqs_hz, n_freq, any_log)) { why = w; return false; }
  return true;
}
static void fmeasure_compact(int n_rows, int32_t n_meas, const ch_fmeasure_spec* specs, std::vector<ch_fmeasure_spec>& sp, std::vector<int>& used) {
  std::vector<int> slot_of(n_rows, -1);
  sp.assign(specs, specs + n_meas);
  auto use = [&](int32_t& r) { if (r < 0) return; if (slot_of[r] < 0) { slot_of[r] = (int)used.size(); used.push_back(r); } r = slot_of[r]; };
  for (ch_fmeasure_spec& m : sp) {
    use(m.s1.row_a); use(m.s1.row_b);
    if (fmeas_uses_s2(m.kind)) { use(m.s2.row_a); use(m.s2.row_b); } else { m.s2 = m.s1; }
  }
}
// frequencies and their log10 (zeros where no spec asks for a LOG axis) -> dst[0 .. 2 n_freq)
static void fmeasure_axes(int32_t n_freq, const double* freqs_hz, const std::vector<ch_fmeasure_spec>& sp, std::vector<double>& ax) {
  bool any_log = false;
  for (const ch_fmeasure_spec& m : sp) any_log = any_log || m.xscale == CH_FX_LOG;
  ax.assign(2 * (size_t)n_freq, 0.0);
  for (int i = 0; i < n_freq; ++i) { ax[i] = freqs_hz[i]; if (any_log) ax[n_freq + i] = std::log10(freqs_hz[i]); }
}
static void fmeasure_launch(hipStream_t st, bool lanes, const FMeasureArgs& a) {
  if (lanes) hipLaunchKernelGGL(fmeasure_lanes_kernel, dim3((unsigned)((a.n_samples + 63) / 64), (unsigned)a.n_meas), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(fmeasure_wave_kernel, dim3((unsigned)a.n_samples, (unsigned)a.n_meas), dim3(64), 0, st, a);
}

static int ch_freq_measure_rows_impl(ch_ctx* ctx, int32_t n_freq, const double* freqs_hz, int32_t n_rows, int32_t n_samples, const double* values, int32_t n_par,
                                     const double* sens, int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status) {
  if (!ctx) return CH_ERR_INVALID;
  ctx->err.clear();
  auto set_err = [&](const std::string& m) { ctx->err = "ch_freq_measure_rows: " + m; };
  auto bad = [&](const std::string& m) { set_err(m); return (int)CH_ERR_INVALID; };
  if (n_meas < 0 || (n_meas > 0 && (!specs || !out_value || !out_status))) return bad("null argument");
  if (n_freq < 1 || n_rows < 1 || n_samples < 1 || !freqs_hz || !values) return bad("no rows to measure");
  if (n_par < 0 || (sens && n_par < 1)) return bad("sensitivity rows without parameters");
  if (out_sens && !sens) return bad("sensitivities asked of rows that carry none");
  { std::string why; if (!fmeasure_check(n_freq, freqs_hz, n_rows, n_meas, specs, why)) return bad(why); }
  if (n_meas == 0) return CH_OK;
  (void)hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int S = n_samples, np = out_sens ? n_par : 0;
  const long nf = n_freq;
  std::vector<ch_fmeasure_spec> sp; std::vector<int> used;
  fmeasure_compact(n_rows, n_meas, specs, sp, used);
  std::vector<double> ax;
  fmeasure_axes(n_freq, freqs_hz, sp, ax);
  // (complex rows: two doubles per element)
  const long chunk = meas_sample_chunk(2 * (long)used.size(), nf, np, S, (double)std::max(1L, env_long(Env::MEASURE_CAP, (long)DENSE_WORK_CAP)));
  // ---- one workspace: axes | specs | values | status | sens | rows | sensitivity rows ----
  const size_t n_out = (size_t)n_meas * S;
  const size_t o_ax = 0, o_sp = o_ax + 2 * (size_t)nf, o_val = o_sp + (sizeof(ch_fmeasure_spec) * (size_t)n_meas + 7) / 8, o_st = o_val + n_out,
               o_sens = o_st + (n_out + 1) / 2, o_rows = o_sens + n_out * (size_t)np, o_srows = o_rows + used.size() * (size_t)nf * (size_t)chunk * 2,
               total = o_srows + used.size() * (size_t)np * (size_t)nf * (size_t)chunk * 2;
  ScopedWorkspace work;
  if (work.alloc(std::max<size_t>(1, total)) != hipSuccess) { set_err("out of device memory for the rows"); return CH_ERR_DEVICE; }
  HIPCHK(hipMemcpy(work.p + o_ax, ax.data(), ax.size() * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(work.p + o_sp, sp.data(), sizeof(ch_fmeasure_spec) * (size_t)n_meas, hipMemcpyHostToDevice));
  const bool lanes = measure_lanes_form(S);
  const size_t cplx = 2 * sizeof(double);
  for (long s0 = 0; s0 < S; s0 += chunk) {
    const long c = std::min<long>(chunk, S - s0);
    FMeasureArgs a; std::memset(&a, 0, sizeof(a));
    a.rows.f = work.p + o_ax; a.rows.ulog = work.p + o_ax + nf; a.rows.nf = nf; a.rows.n_par = np;
    a.rows.H = work.p + o_rows; a.rows.ldH = c;
    for (size_t u = 0; u < used.size(); ++u)
      HIPCHK(hipMemcpy2D(work.p + o_rows + u * (size_t)nf * c * 2, (size_t)c * cplx, values + ((size_t)used[u] * nf * S + s0) * 2, (size_t)S * cplx, (size_t)c * cplx, (size_t)nf,
                         hipMemcpyHostToDevice));
    if (np > 0) {
      a.rows.dH = work.p + o_srows; a.rows.ldS = c;
      for (size_t u = 0; u < used.size(); ++u) for (int k = 0; k < np; ++k)
        HIPCHK(hipMemcpy2D(work.p + o_srows + (u * np + k) * (size_t)nf * c * 2, (size_t)c * cplx, sens + (((size_t)used[u] * n_par + k) * nf * S + s0) * 2, (size_t)S * cplx,
                           (size_t)c * cplx, (size_t)nf, hipMemcpyHostToDevice));
    }
    a.specs = (const ch_fmeasure_spec*)(work.p + o_sp); a.n_meas = n_meas; a.n_samples = (int)c;
    a.value = work.p + o_val + s0; a.status = (int*)(work.p + o_st) + s0; a.sens = np > 0 ? work.p + o_sens + s0 : nullptr; a.ldo = S;
    fmeasure_launch(st, lanes, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the next chunk's copies reuse the row buffers
  }
  HIPCHK(hipMemcpy(out_value, work.p + o_val, n_out * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out_status, work.p + o_st, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (np > 0) HIPCHK(hipMemcpy(out_sens, work.p + o_sens, n_out * (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
  return CH_OK;
}

static int ch_ac_measure_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq, const double* freqs_hz,
                              int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status, int32_t* sample_status, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  auto set_err = [&](const std::string& m) { c->set_err("ch_ac_measure: " + m); };
  auto bad = [&](const std::string& m) { set_err(m); return (int)CH_ERR_INVALID; };
  if (n_meas < 1 || !specs || !out_value || !out_status) return bad("at least one measure and its output arrays");
  if (n_par < 0 || (n_par > 0 && !out_sens)) return bad("parameters without an array for the sensitivities");
  if (n_freq < 1 || !freqs_hz) return bad("at least one frequency");
  const Analysis& A = c->desc.A;
  { std::string why; if (!fmeasure_check(n_freq, freqs_hz, A.n_mna, n_meas, specs, why)) return bad(why); }
  // ---- the analysis, on the device ----
  AcSensDevice D; ch_stats st0; hclock::time_point t0;
  int rc = n_par > 0 ? acsens_device_solve(c, "ch_ac_measure", o, n_par, slot_ids, so, n_freq, freqs_hz, out_sens, nullptr, sample_status, D)
                     : ac_device_solve(c, o, n_freq, freqs_hz, st0, t0, stats);
  if (rc != CH_OK) return rc;
  const int S = c->tab.S, nu = A.n_unk;
  if (n_par == 0 && sample_status) for (int s = 0; s < S; ++s) sample_status[s] = CH_OK;
  hipStream_t stream = c->ctx->stream;
  // ---- the rows the specs name: MNA index -> unknown, 0 or NaN (the rule of acsens_expand_mna) ----
  std::vector<ch_fmeasure_spec> sp; std::vector<int> used;
  fmeasure_compact(A.n_mna, n_meas, specs, sp, used);
  std::vector<int> src(used.size());
  for (size_t r = 0; r < used.size(); ++r) {
    const int m = used[r];
    int u;
    if (m < A.n_nodes) { u = A.node_unknown[m + 1]; if (u < 0) u = -1; }
    else { u = A.branch_unknown[m - A.n_nodes]; if (u < 0) u = -2; }
    if (u >= nu) { set_err("internal: an unknown out of range"); return CH_ERR_INTERNAL; }
    src[r] = u;
  }
  std::vector<double> ax;
  fmeasure_axes(n_freq, freqs_hz, sp, ax);
  const long nf = n_freq;
  const size_t n_out = (size_t)n_meas * S, n_used = used.size();
  const size_t o_ax = 0, o_sp = o_ax + 2 * (size_t)nf, o_src = o_sp + (sizeof(ch_fmeasure_spec) * (size_t)n_meas + 7) / 8, o_val = o_src + (n_used + 1) / 2, o_st = o_val + n_out,
               o_sens = o_st + (n_out + 1) / 2, o_rows = o_sens + n_out * (size_t)n_par, o_srows = o_rows + n_used * (size_t)nf * S * 2,
               total = o_srows + n_used * (size_t)n_par * (size_t)nf * S * 2;
  ScopedWorkspace work;
  if (work.alloc(std::max<size_t>(1, total)) != hipSuccess) { set_err("out of device memory for the rows"); return CH_ERR_DEVICE; }
  HIPCHK(hipMemcpyAsync(work.p + o_ax, ax.data(), ax.size() * sizeof(double), hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(work.p + o_sp, sp.data(), sizeof(ch_fmeasure_spec) * (size_t)n_meas, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyAsync(work.p + o_src, src.data(), sizeof(int) * n_used, hipMemcpyHostToDevice, stream));
  const int* d_skip = n_par > 0 ? c->sens.d_skip.p : nullptr;
  FGatherArgs g; std::memset(&g, 0, sizeof(g));
  g.x = c->ac.d_xac.p; g.z = n_par > 0 ? c->sens.d_xac_sens.p : nullptr; g.src = (const int*)(work.p + o_src); g.n_used = (int)n_used; g.skip = d_skip;
  g.S = S; g.n_freq = n_freq; g.n_unk = nu; g.n_par = n_par; g.H = work.p + o_rows; g.dH = work.p + o_srows;
  hipLaunchKernelGGL(fmeasure_gather_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)n_freq, (unsigned)n_used), dim3(64), 0, stream, g);
  HIPCHK(hipGetLastError());
  FMeasureArgs a; std::memset(&a, 0, sizeof(a));
  a.rows.f = work.p + o_ax; a.rows.ulog = work.p + o_ax + nf; a.rows.nf = nf; a.rows.n_par = n_par;
  a.rows.H = work.p + o_rows; a.rows.ldH = S; a.rows.dH = n_par > 0 ? work.p + o_srows : nullptr; a.rows.ldS = S;
  a.specs = (const ch_fmeasure_spec*)(work.p + o_sp); a.n_meas = n_meas; a.n_samples = S;
  a.value = work.p + o_val; a.status = (int*)(work.p + o_st); a.sens = n_par > 0 ? work.p + o_sens : nullptr; a.ldo = S; a.skip = d_skip;
  fmeasure_launch(stream, measure_lanes_form(S), a);
  HIPCHK(hipGetLastError());
  int fail = 0;
  HIPCHK(hipMemcpyAsync(out_value, work.p + o_val, n_out * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(out_status, work.p + o_st, n_out * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  if (n_par > 0) HIPCHK(hipMemcpyAsync(out_sens, work.p + o_sens, n_out * (size_t)n_par * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipMemcpyAsync(&fail, n_par > 0 ? c->sens.d_fail.p : c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (n_par > 0) return acsens_finish(c, D, n_par, n_freq, 2, fail, stats);
  return ac_finish(c, "AC analysis", st0, t0, n_freq, 4, fail, stats);
}
}  // extern "C++"
