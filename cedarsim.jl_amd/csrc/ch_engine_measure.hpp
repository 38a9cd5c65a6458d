// ch_engine_measure.hpp — waveform measurements over a finished transient (ch_measure_rows, ch_result_measure): both are thin callers
// of measure_run, which checks the specs (meas_spec_check, before anything is uploaded), brings the rows the specs name to the device
// — or reads a device-stepper result's rows where they still are — and launches one of the two kernels of ch_measure_kernels.hpp per
// sample chunk: lanes per sample from 64 samples up, the time split below (measure_lanes_form; CEDARHIP_MEASURE_SPLIT overrides).
// The form is chosen by the call's sample count, never by a chunk's, so a sample's result does not depend on its chunk.
// Included by ch_engine.hip behind ch_engine_transens.hpp.
#pragma once

extern "C++" {   // (included inside the extern "C" block of ch_engine.hip)

struct MeasureInput {
  long nt = 0; const double* times = nullptr; const int32_t* pts = nullptr;
  int n_rows = 0, S = 0;
  const double* values = nullptr;       // host [n_rows][nt][S]
  int n_par = 0; const double* sens = nullptr;   // host [n_rows][n_par][nt][S], or null
  const double* dev_values = nullptr;   // the same values in HBM, or null
};

// the kernel form of a waveform or frequency-domain measurement over S samples: a lane per sample from 64 samples up, else a wavefront
// per sample; CEDARHIP_MEASURE_SPLIT = lanes | time overrides, any other value leaves the rule alone
static bool measure_lanes_form(int S) {
  const char* split = env_get(Env::MEASURE_SPLIT);
  return (split && std::strcmp(split, "lanes") == 0) || (!(split && std::strcmp(split, "time") == 0) && S >= 64);
}

static int measure_run(ch_ctx* ctx, const char* who, const MeasureInput& in, int32_t n_meas, const ch_measure_spec* specs, double* out_value, double* out_sens,
                       int32_t* out_status) {
  if (!ctx) return CH_ERR_INVALID;
  ctx->err.clear();
  auto set_err = [&](const std::string& m) { ctx->err = std::string(who) + ": " + m; };
  auto bad = [&](const std::string& m) { set_err(m); return (int)CH_ERR_INVALID; };
  if (n_meas < 0 || (n_meas > 0 && (!specs || !out_value || !out_status))) return bad("null argument");
  if (in.nt < 1 || in.n_rows < 1 || in.S < 1 || !in.times || (!in.values && !in.dev_values)) return bad("no rows to measure");
  if (in.n_par < 0 || (in.sens && in.n_par < 1)) return bad("sensitivity rows without parameters");
  if (out_sens && !in.sens) return bad("sensitivities asked of rows that carry none (a result of ch_tran_sens has them)");
  for (long i = 0; i < in.nt; ++i) {
    if (!std::isfinite(in.times[i]) || (i > 0 && in.times[i] < in.times[i - 1])) return bad("times must be finite and non-decreasing");
    if (in.pts && (in.pts[i] < 0 || in.pts[i] > MEAS_MAX_PTS)) return bad("dense point counts must lie in 0.." + std::to_string(MEAS_MAX_PTS));
  }
  for (int k = 0; k < n_meas; ++k) if (const char* why = meas_spec_check(specs[k], in.n_rows)) return bad("measure " + std::to_string(k) + ": " + why);
  if (n_meas == 0) return CH_OK;
  (void)hipSetDevice(ctx->device);
  hipStream_t st = ctx->stream;
  const int S = in.S, np = out_sens ? in.n_par : 0;
  const long nt = in.nt;
  // ---- the rows the specs name, in order of first use; a device-stepper result's rows are read where they are ----
  const bool in_place = in.dev_values != nullptr && np == 0;
  if (!in_place && !in.values) return bad("the rows are on the device only, and sensitivities need them on the host");
  std::vector<int> slot_of(in.n_rows, -1), used;
  std::vector<ch_measure_spec> sp(specs, specs + n_meas);
  auto use = [&](int32_t& r) { if (r < 0) return; if (slot_of[r] < 0) { slot_of[r] = (int)used.size(); used.push_back(r); } if (!in_place) r = slot_of[r]; };
  for (ch_measure_spec& m : sp) {
    use(m.s1.row_a); use(m.s1.row_b);
    if (meas_uses_s2(m.kind)) { use(m.s2.row_a); use(m.s2.row_b); } else { m.s2.row_a = 0; m.s2.row_b = -1; }
  }
  const long chunk = in_place ? (long)S : meas_sample_chunk((long)used.size(), nt, np, S, (double)std::max(1L, env_long(Env::MEASURE_CAP, (long)DENSE_WORK_CAP)));
  // ---- one workspace: times | dense points | specs | values | status | sens | state rows | sensitivity rows ----
  const size_t n_out = (size_t)n_meas * S;
  const size_t o_t = 0, o_pts = o_t + (size_t)nt, o_sp = o_pts + ((size_t)nt + 1) / 2, o_val = o_sp + (sizeof(ch_measure_spec) * (size_t)n_meas + 7) / 8,
               o_st = o_val + n_out, o_sens = o_st + (n_out + 1) / 2, o_rows = o_sens + n_out * (size_t)np,
               o_srows = o_rows + (in_place ? 0 : used.size() * (size_t)nt * (size_t)chunk), total = o_srows + used.size() * (size_t)np * (size_t)nt * (size_t)chunk;
  ScopedWorkspace work;
  if (work.alloc(std::max<size_t>(1, total)) != hipSuccess) { set_err("out of device memory for the rows"); return CH_ERR_DEVICE; }
  HIPCHK(hipMemcpy(work.p + o_t, in.times, (size_t)nt * sizeof(double), hipMemcpyHostToDevice));
  if (in.pts) HIPCHK(hipMemcpy(work.p + o_pts, in.pts, (size_t)nt * sizeof(int32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(work.p + o_sp, sp.data(), sizeof(ch_measure_spec) * (size_t)n_meas, hipMemcpyHostToDevice));
  const bool lanes = measure_lanes_form(S);
  for (long s0 = 0; s0 < S; s0 += chunk) {
    const long c = std::min<long>(chunk, S - s0);
    MeasureArgs a; std::memset(&a, 0, sizeof(a));
    a.rows.t = work.p + o_t; a.rows.pts = in.pts ? (const int32_t*)(work.p + o_pts) : nullptr; a.rows.nt = nt; a.rows.n_par = np;
    if (in_place) { a.rows.V = in.dev_values + s0; a.rows.ldV = S; }
    else {
      a.rows.V = work.p + o_rows; a.rows.ldV = c;
      for (size_t u = 0; u < used.size(); ++u)
        HIPCHK(hipMemcpy2D(work.p + o_rows + u * (size_t)nt * c, (size_t)c * sizeof(double), in.values + (size_t)used[u] * nt * S + s0, (size_t)S * sizeof(double),
                           (size_t)c * sizeof(double), (size_t)nt, hipMemcpyHostToDevice));
    }
    if (np > 0) {
      a.rows.Sn = work.p + o_srows; a.rows.ldS = c;
      for (size_t u = 0; u < used.size(); ++u) for (int k = 0; k < np; ++k)
        HIPCHK(hipMemcpy2D(work.p + o_srows + (u * np + k) * (size_t)nt * c, (size_t)c * sizeof(double), in.sens + ((size_t)used[u] * in.n_par + k) * nt * S + s0,
                           (size_t)S * sizeof(double), (size_t)c * sizeof(double), (size_t)nt, hipMemcpyHostToDevice));
    }
    a.specs = (const ch_measure_spec*)(work.p + o_sp); a.n_meas = n_meas; a.n_samples = (int)c;
    a.value = work.p + o_val + s0; a.status = (int*)(work.p + o_st) + s0; a.sens = np > 0 ? work.p + o_sens + s0 : nullptr; a.ldo = S;
    if (lanes) hipLaunchKernelGGL(measure_lanes_kernel, dim3((unsigned)((c + 63) / 64), (unsigned)n_meas), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(measure_wave_kernel, dim3((unsigned)c, (unsigned)n_meas), dim3(64), 0, st, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // the next chunk's copies reuse the row buffers
  }
  HIPCHK(hipMemcpy(out_value, work.p + o_val, n_out * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out_status, work.p + o_st, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (np > 0) HIPCHK(hipMemcpy(out_sens, work.p + o_sens, n_out * (size_t)np * sizeof(double), hipMemcpyDeviceToHost));
  return CH_OK;
}

static int ch_measure_rows_impl(ch_ctx* ctx, int64_t n_times, const double* times, const int32_t* dense_points, int32_t n_rows, int32_t n_samples, const double* values,
                                int32_t n_par, const double* sens, int32_t n_meas, const ch_measure_spec* specs, double* out_value, double* out_sens, int32_t* out_status) {
  MeasureInput in;
  in.nt = (long)n_times; in.times = times; in.pts = dense_points; in.n_rows = n_rows; in.S = n_samples; in.values = values; in.n_par = n_par; in.sens = sens;
  return measure_run(ctx, "ch_measure_rows", in, n_meas, specs, out_value, out_sens, out_status);
}

static int ch_result_measure_impl(const ch_result* r, int32_t n_meas, const ch_measure_spec* specs, double* out_value, double* out_sens, int32_t* out_status) {
  MeasureInput in;
  in.nt = (long)r->times.size(); in.times = r->times.data(); in.pts = r->pts.size() == r->times.size() ? r->pts.data() : nullptr;
  in.n_rows = r->n_obs; in.S = r->S;
  const size_t n = (size_t)r->n_obs * r->times.size() * (size_t)r->S;
  in.values = (n > 0 && r->values.size() == n) ? r->values.data() : nullptr;
  in.dev_values = (n > 0 && r->dev_n == (int64_t)n) ? r->dev_values : nullptr;
  in.n_par = r->n_par; in.sens = (r->n_par > 0 && r->sens.size() == n * (size_t)r->n_par) ? r->sens.data() : nullptr;
  if (!in.sens) in.n_par = 0;
  return measure_run(r->ctx, "ch_result_measure", in, n_meas, specs, out_value, out_sens, out_status);
}
}  // extern "C++"
