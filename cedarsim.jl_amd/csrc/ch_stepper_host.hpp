// ch_stepper_host.hpp — the host side of time stepping without any HIP: source waveforms and their break points, the
// variable-coefficient BDF / extrapolation weights, and the step controller (StepControl) that ch_engine.hip drives with one
// Newton launch per attempt.  HIP-free like ch_sparse_host.hpp, so the policy runs under ASan/UBSan on the CPU
// (tests/host_stepper_fuzz.cpp).  The device-resident stepper (ch_persist.hpp) and the oracle keep their own copies of the
// same policy; the GPU tests assert equal accepted / rejected / iteration counts between them, so the arithmetic here is
// not to be "simplified": expression order is part of the contract.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "ch_analysis.hpp"
#include "ch_env.hpp"

namespace chip {

// ---- source waveforms (src/spectre_env.jl:15-21, :43-69, :153-166, :169-176) ----
inline double pwl_at_time(const double* ts, const double* ys, int n, double t) {
  if (n == 0) return 0.0;
  int i = (int)(std::lower_bound(ts, ts + n, t) - ts) + 1;
  if (i <= n && ts[i - 1] == t) ++i;
  if (i <= 1) return ys[0];
  if (i > n) return ys[n - 1];
  if (ys[i - 2] == ys[i - 1]) return ys[i - 1];
  if (ts[i - 1] == ts[i - 2]) return 0.5 * (ys[i - 2] + ys[i - 1]);
  return ys[i - 2] + (t - ts[i - 2]) * ((ys[i - 1] - ys[i - 2]) / (ts[i - 1] - ts[i - 2]));
}
inline double sind(double deg) { return std::sin(std::fmod(deg, 360.0) * (3.14159265358979323846 / 180.0)); }
// mode 0 :dcop, 1 :tran at t, 2 :tranop (t = 0)
inline double source_value(const HSource& s, const double* par, double dc, double t, int mode) {
  if (mode == 0) return dc;
  if (mode == 2) t = 0.0;
  switch (s.kind) {
    case CH_SRC_DC: return par[0];
    case CH_SRC_PWL: return pwl_at_time(s.ts.data(), s.ys.data(), (int)s.ts.size(), t);
    case CH_SRC_PULSE: {
      const double td = par[2], tr = par[3], tf = par[4], pw = par[5], per = par[6];
      const double ts[4] = {td, td + tr, td + tr + pw, td + tr + pw + tf}, ys[4] = {par[0], par[1], par[1], par[0]};
      return pwl_at_time(ts, ys, 4, std::isfinite(per) ? std::fmod(t, per) : t);
    }
    case CH_SRC_SIN: {
      const double vo = par[0], va = par[1], f = par[2], td = par[3], th = par[4], ph = par[5], nc = par[6];
      if (td < t && t < nc / f) return vo + va * std::exp(-(t - td) * th) * sind(360.0 * f * (t - td) + ph);
      return vo + va * sind(ph);
    }
  }
  return 0.0;
}
inline void source_breakpoints(const HSource& s, const double* par, double t0, double t1, std::vector<double>& out) {
  if (s.kind == CH_SRC_PWL) { for (double t : s.ts) if (t > t0 && t < t1) out.push_back(t); }
  else if (s.kind == CH_SRC_PULSE) {
    const double td = par[2], tr = par[3], tf = par[4], pw = par[5], per = par[6];
    const double c[4] = {td, td + tr, td + tr + pw, td + tr + pw + tf};
    if (!std::isfinite(per) || per <= 0) { for (double t : c) if (t > t0 && t < t1) out.push_back(t); }
    else {
      long k0 = std::max(0L, (long)std::floor(t0 / per) - 1);
      for (long k = k0; k * per < t1 && (k - k0) < 10000000; ++k) {
        for (double tc : c) { double t = tc + k * per; if (t > t0 && t < t1) out.push_back(t); }
        if (k >= 1 && k * per > t0 && k * per < t1) out.push_back(k * per);  // wrap of `t mod period` may jump
      }
    }
  } else if (s.kind == CH_SRC_SIN) {
    const double te = par[6] / par[2];
    if (par[3] > t0 && par[3] < t1) out.push_back(par[3]);
    if (std::isfinite(te) && te > t0 && te < t1) out.push_back(te);
  }
}

// Does the source VALUE jump at t, or is t only a corner (slope discontinuity)?  Same rule as oracle.cpp source_jumps_at.
inline bool source_jumps_at(const HSource& s, const double* par, double t) {
  double amp = 0.0;
  if (s.kind == CH_SRC_PWL) for (double y : s.ys) amp = std::max(amp, std::fabs(y));
  else if (s.kind == CH_SRC_PULSE) amp = std::max(std::fabs(par[0]), std::fabs(par[1]));
  else if (s.kind == CH_SRC_SIN) amp = std::fabs(par[0]) + std::fabs(par[1]);
  const double a = source_value(s, par, 0.0, std::nextafter(t, -INFINITY), 1), b = source_value(s, par, 0.0, t, 1);
  return std::fabs(a - b) > 1e-9 * amp;
}

// (time, code) of one source's break points in (t0, t1): code < 0 = the value jumps, else the length of the segment that starts there
inline void source_breakpoint_codes(const HSource& s, const double* par, double t0, double t1, std::vector<std::pair<double, double>>& out) {
  const bool restart_all = env_on(Env::BP_RESTART_ALL);   // the policy of rounds 1-2 (A/B switch; read per call: the tests flip it)
  std::vector<double> own;
  source_breakpoints(s, par, t0, t1, own);
  std::sort(own.begin(), own.end());
  for (size_t j = 0; j < own.size(); ++j) {
    const double seg = (j + 1 < own.size() ? own[j + 1] : t1) - own[j];
    out.emplace_back(own[j], (restart_all || source_jumps_at(s, par, own[j])) ? -1.0 : seg);
  }
}
// sorted unique times with merged codes (a jump wins, otherwise the shortest segment); t1 closes the list
inline void merge_breakpoints(std::vector<std::pair<double, double>>& pts, double t1, std::vector<double>& bps, std::vector<double>& bpc) {
  pts.emplace_back(t1, -1.0);
  std::sort(pts.begin(), pts.end());
  bps.clear(); bpc.clear();
  for (const auto& pt : pts) {
    if (!bps.empty() && bps.back() == pt.first) { bpc.back() = (bpc.back() < 0 || pt.second < 0) ? -1.0 : std::min(bpc.back(), pt.second); continue; }
    bps.push_back(pt.first); bpc.push_back(pt.second);
  }
}

// Break points of the sources `only` (null: all of them) over n_sets parameter sets, each with its code: < 0 = some source VALUE
// jumps there (the integrator restarts at order 1 behind it); >= 0 = a continuous corner (landed on exactly, stepped over with the
// history kept — IDA's treatment of `tstops`, src/spectre_env.jl:71-77) and the code is the length of the shortest source segment
// that starts there (the first step behind the corner is capped at a tenth of it).  A source is asked only about its own times:
// linear in the number of points.  Serves the whole circuit's list and every workgroup's own (per-block steps).
inline void collect_breakpoints(const std::vector<HSource>& srcs, const std::vector<double>& src_par, int n_sets, double t0, double t1,
                                std::vector<double>& bps, std::vector<double>& bpc, const std::vector<int>* only = nullptr) {
  const size_t nsrc = srcs.size(), n = only ? only->size() : nsrc;
  std::vector<std::pair<double, double>> pts;
  for (int s = 0; s < n_sets; ++s) for (size_t q = 0; q < n; ++q) {
    const size_t i = only ? (size_t)(*only)[q] : q;
    source_breakpoint_codes(srcs[i], &src_par[((size_t)s * nsrc + i) * CH_SRC_NPAR], t0, t1, pts);
  }
  merge_breakpoints(pts, t1, bps, bpc);
}

// ---- the resolved request of one transient: built once by tran_solve, read by both steppers ----
struct TranPlan {
  double t0 = 0, t1 = 0; int kmax = 1; double dtmin = 0, dtmax = 0; int max_steps = 0, nmaxit = 0;
  std::vector<double> bps, bpc;            // merged break points (closed by t1) and their codes (collect_breakpoints)
  const ch_tran_opts* o = nullptr;         // the caller's options: tolerances, dt0, the output grid, the stepper wishes
};
// the default rules, once: order 1..5, dtmax a tenth of the span, dtmin 1e-15 of it, Sundials.jl's default maxiters of
// solve(prob, IDA()) steps, 10 Newton iterations per attempt.  t1 > t0: check_tran_opts
inline TranPlan resolve_tran_plan(double t0, double t1, const ch_tran_opts& o) {
  TranPlan p;
  const double span = t1 - t0;
  p.t0 = t0; p.t1 = t1; p.o = &o;
  p.kmax = std::min(5, std::max(1, o.max_order));
  p.dtmax = o.dtmax > 0 ? o.dtmax : span / 10.0; p.dtmin = o.dtmin > 0 ? o.dtmin : 1e-15 * span;
  p.max_steps = o.max_steps > 0 ? o.max_steps : 100000; p.nmaxit = o.newton_maxiters > 0 ? o.newton_maxiters : 10;
  return p;
}
// Rows of the device stepper's output buffer: the grid and one more with saveat; otherwise every step the transient may take,
// but at least 1024 rows and at most 2^20 or 256 MB of them.  `forced` (CEDARHIP_PERSIST_MAXROWS; null: none) replaces the rule
// where there is no grid: a test hook that forces the drain-and-resume path.
inline long long persist_max_rows(int n_saveat, int max_steps, size_t row_doubles, const long* forced) {
  if (n_saveat > 0) return (long long)n_saveat + 1;
  if (forced) return std::max(2L, *forced);
  return std::min<long long>((long long)max_steps + 2, std::max<long long>(1024, std::min<long long>(1 << 20, (long long)((256u << 20) / (row_doubles * sizeof(double))))));
}

// one Newton solve's iterations into the statistics: every iteration is one residual, one Jacobian, one factorisation, one solve
inline void add_newton_iters(ch_stats& s, long long iters, long long block_iters) {
  s.n_block_iters += block_iters; s.nnonliniter += iters; s.nf += iters; s.njacs += iters; s.nfactors += iters; s.nsolve += iters;
}

// variable-coefficient BDF helpers: tau[0] = t_new, tau[1..] history (newest first)
inline void bdf_coeffs(const double* tau, int k, double* alpha) {
  double a0 = 0;
  for (int m = 1; m <= k; ++m) a0 += 1.0 / (tau[0] - tau[m]);
  alpha[0] = a0;
  for (int j = 1; j <= k; ++j) {
    double num = 1, den = 1;
    for (int m = 1; m <= k; ++m) if (m != j) num *= (tau[0] - tau[m]);
    for (int m = 0; m <= k; ++m) if (m != j) den *= (tau[j] - tau[m]);
    alpha[j] = num / den;
  }
}
inline void extrap_weights(const double* tau, int np, double* w) {
  for (int j = 1; j <= np; ++j) { double v = 1; for (int i = 1; i <= np; ++i) if (i != j) v *= (tau[0] - tau[i]) / (tau[j] - tau[i]); w[j] = v; }
}

// ---- host step controller ------------------------------------------------------------------------------------------------
constexpr int NSLOT = 8;  // 7 history points + 1 candidate
constexpr double FIRST_STEP_FRAC = 1e-3;   // PersistArgs::first_frac is filled from this constant

// The first step of a transient and of every restart behind a jump: a fiftieth of the way to the next break point at most,
// then a thousandth of that (the order-1 start has no error estimate to protect it).  `h` is the step that would be taken
// otherwise.  The single host definition; the device stepper's own is in ch_persist.hpp.
inline double first_step(double h, double t, double next_bp, double dtmin) {
  return std::max(10 * dtmin, std::min(h, (next_bp - t) / 50.0) * FIRST_STEP_FRAC);
}
inline double start_step(double dt0, double t0, double t1, double dtmin, double dtmax, double first_bp) {
  const double span = t1 - t0;
  const double h = dt0 > 0 ? dt0 : std::min(dtmax, 1e-3 * span);
  return first_step(h, t0, first_bp, dtmin);
}

// CEDARHIP_STEPPER / ch_tran_opts.stepper -> CH_STEPPER_*: the option wins unless it is AUTO.  `device_known` = false is the
// torn-form call site, which only asks "host or not": "device" maps to AUTO there, with the same effect (want != HOST).
inline int resolve_stepper(int opt, const char* ev, bool device_known = true) {
  if (opt != CH_STEPPER_AUTO || !ev) return opt;
  if (std::strcmp(ev, "host") == 0) return CH_STEPPER_HOST;
  return (device_known && std::strcmp(ev, "device") == 0) ? CH_STEPPER_DEVICE : CH_STEPPER_AUTO;
}

// rows [row][obs][sample] -> the result's layout [obs][time][sample], rows row0 .. row0+rows-1 of nt
inline void rows_to_obs_major(const double* rows_in, size_t rows, size_t row0, size_t nt, int n_obs, int S, double* values) {
  for (size_t r = 0; r < rows; ++r) for (int ob = 0; ob < n_obs; ++ob)
    std::copy(rows_in + (r * n_obs + ob) * S, rows_in + (r * n_obs + ob + 1) * S, values + ((size_t)ob * nt + row0 + r) * S);
}

// Launch statistics of one engine call: every timing and launch counter of a circuit.  The Newton launcher times one launch in
// `time_every` with HIP events (device_ms sums those n_timed launches only); the device stepper's launches are timed exactly.
struct LaunchStats {
  double device_ms = 0; long n_launch = 0, n_timed = 0;              // fused / sparse Newton launches; the sampled ones
  double prof_launch = 0, prof_wait = 0, prof_reduce = 0;            // host seconds inside run_newton (CEDARHIP_HOST_PROFILE)
  double persist_ms = 0; long persist_launches = 0; long long persist_attempts = 0; double persist_barrier_s = 0;   // device stepper
  double dc_device_ms = 0; long dc_launches = 0, dc_timed = 0; long long dc_block_iters = 0;   // snapshot behind the initialisation
  void reset() { *this = LaunchStats(); }
  void end_of_dc(long long block_iters) { dc_device_ms = device_ms; dc_launches = n_launch; dc_timed = n_timed; dc_block_iters = block_iters; }
  static double scaled_seconds(double ms, long launches, long timed) { return timed > 0 ? ms * 1e-3 * (double)launches / (double)timed : 0.0; }
  // device_seconds: sampled launches scaled + the persistent launches (exact); step_kernel_*: the launches behind end_of_dc()
  void fill(ch_stats& s) const {
    s.device_seconds = scaled_seconds(device_ms, n_launch, n_timed) + persist_ms * 1e-3;
    const bool dev = persist_launches > 0;
    s.step_kernel_launches = dev ? persist_launches : n_launch - dc_launches;
    s.step_kernel_seconds = dev ? persist_ms * 1e-3 : scaled_seconds(device_ms - dc_device_ms, n_launch - dc_launches, n_timed - dc_timed);
  }
};

// coefficient block of one attempt, copied into NewtonArgs by the launcher.  It lives as long as the controller: fields an
// attempt does not use (nkm1 == 0, nkp1 == 0, alpha above k) keep what an earlier attempt left there.
struct StepCoeffs {
  int k = 0, npred = 0, nkm1 = 0, nkp1 = 0;
  double alpha[8] = {0}, wpred[8] = {0}, wkm1[8] = {0}, wkp1[8] = {0};
  double ck = 0, ckm1 = 0, ckp1 = 0;
  int hist_slot[8] = {0}, cand_slot = 0;
};

// Variable-order variable-step BDF controller in the manner of IDA (the job IDA does in the reference, src/sweeps.jl:456).
// One attempt: plan() -> [Newton solve] -> on_convergence_failure() | on_error_test_failure() | on_accept() + select_next().
struct StepControl {
  const double t1, dtmin, dtmax; const int kmax;
  const std::vector<double>& bps; const std::vector<double>& bpc;   // break points (closed by t1) and their codes (merge_breakpoints)
  // ---- state ----
  double t, h;
  int k = 1, nhist = 1, steps_at_order = 0;
  bool reset_rate = true;  // convergence rates unknown at the start and after every restart
  size_t ibp = 0;
  // ring bookkeeping: order[] lists slots newest-first
  int order[NSLOT]; double htime[NSLOT] = {0};
  // ---- the attempt planned last ----
  double tn = 0, hh = 0, tb_code = -1.0;
  bool hit_bp = false, lte = false, try_up = false;
  int kk = 1, np = 1, nh = 1;
  StepCoeffs c;

  StepControl(double t0, double t1_, double dt0, double dtmin_, double dtmax_, int kmax_, const std::vector<double>& bps_, const std::vector<double>& bpc_)
      : t1(t1_), dtmin(dtmin_), dtmax(dtmax_), kmax(kmax_), bps(bps_), bpc(bpc_), t(t0), h(start_step(dt0, t0, t1_, dtmin_, dtmax_, bps_[0])) {
    for (int i = 0; i < NSLOT; ++i) order[i] = i;
    htime[0] = t0;
  }
  explicit StepControl(const TranPlan& p) : StepControl(p.t0, p.t1, p.o->dt0, p.dtmin, p.dtmax, p.kmax, p.bps, p.bpc) {}   // refers to the plan's lists: it outlives the controller
  bool tb_jump() const { return tb_code < 0; }
  int dense_points() const { return std::min(kk, nh) + 1; }   // newest points the accepted step's dense-output polynomial runs through

  // target time, orders and coefficients of the next attempt; CH_ERR_DTMIN when the step would fall below dtmin
  int plan() {
    while (ibp < bps.size() && bps[ibp] <= t * (1 + 1e-15) + 1e-300) ++ibp;
    const double tb = ibp < bps.size() ? bps[ibp] : t1;
    tb_code = ibp < bps.size() ? bpc[ibp] : -1.0;
    hit_bp = false;
    tn = t + h;
    if (tn >= tb - 1e-3 * h) { tn = tb; hit_bp = true; }
    hh = tn - t;
    if (hh < dtmin) return CH_ERR_DTMIN;
    nh = nhist; kk = std::min(k, nh); np = std::min(kk + 1, nh);
    double tau[9];
    tau[0] = tn; for (int j = 0; j < nh && j < 7; ++j) tau[j + 1] = htime[j];
    extrap_weights(tau, np, c.wpred); c.npred = np;
    bdf_coeffs(tau, kk, c.alpha); c.k = kk;
    lte = np >= kk + 1;
    c.ck = lte ? hh / (tn - tau[kk + 1]) : 0.0;
    c.nkm1 = 0; c.nkp1 = 0; c.ckm1 = 0; c.ckp1 = 0;
    try_up = lte && kk < kmax && nh >= kk + 2 && steps_at_order + 1 >= kk + 1;
    if (lte && kk > 1) { extrap_weights(tau, kk, c.wkm1); c.nkm1 = kk; c.ckm1 = hh / (tn - tau[kk]); }
    if (try_up) { extrap_weights(tau, kk + 2, c.wkp1); c.nkp1 = kk + 2; c.ckp1 = hh / (tn - tau[kk + 2]); }
    for (int j = 0; j < 7; ++j) c.hist_slot[j] = order[std::min(j, nh - 1)];
    c.cand_slot = order[NSLOT - 1];
    return CH_OK;
  }
  // landing on a break point uses the sources' left limit there; the jump (if any) is crossed by the restart step
  double source_time() const { return hit_bp ? std::nextafter(tn, -INFINITY) : tn; }

  void on_convergence_failure() {
    reset_rate = true;
    h = hh * 0.25; k = 1; steps_at_order = 0;
    if (nhist > 2) nhist = 2;
  }
  void on_error_test_failure(double errk) {
    // IDA-style: aim at half the tolerance after a failed error test, shrink by at most 4x
    const double fac = 0.9 * std::pow(2.0 * errk + 1e-4, -1.0 / (kk + 1));
    h = hh * std::min(0.9, std::max(0.25, fac));
    steps_at_order = 0;
  }
  // accept: the candidate slot becomes the newest history point
  void on_accept() {
    reset_rate = false;
    int cand = order[NSLOT - 1];
    for (int j = NSLOT - 1; j > 0; --j) { order[j] = order[j - 1]; htime[j] = htime[j - 1]; }
    order[0] = cand; htime[0] = tn; nhist = std::min(nhist + 1, kmax + 2);
  }
  // weights of the accepted step's dense-output polynomial at ts (a saveat point inside the step): ww[1..m] go with order[0..m-1]
  int dense_weights(double ts, double* ww) const {
    double tt[9]; const int m = dense_points();
    tt[0] = ts; for (int j = 0; j < m; ++j) tt[j + 1] = htime[j];
    extrap_weights(tt, m, ww);
    return m;
  }
  // order / step selection behind an accepted step, then the corner and jump handling when it landed on a break point
  void select_next(double errk, double errkm1, double errkp1) {
    const double fac_k = std::pow(2.0 * errk + 1e-4, -1.0 / (kk + 1));  // puts the error at half the tolerance
    double best = fac_k; int knew = kk;
    if (lte) {
      ++steps_at_order;
      if (kk > 1) { const double f = std::pow(2.0 * errkm1 + 1e-4, -1.0 / kk); if (f > best) { best = f; knew = kk - 1; } }
      if (try_up) { const double f = std::pow(2.0 * errkp1 + 1e-4, -1.0 / (kk + 2)); if (f > 1.1 * best) { best = f; knew = kk + 1; } }
    } else knew = 1;
    if (knew != kk) steps_at_order = 0;
    k = knew;
    if (best > 1.0 && best < 1.2) best = 1.0;  // dead band: keep h when the suggested change is small
    h = std::min(dtmax, hh * std::min(kk == 1 ? 10.0 : 2.0, std::max(0.5, best)));
    t = tn;
    if (hit_bp && t < t1 && !tb_jump()) {   // continuous corner: history and order are kept, the first step behind it is capped (oracle.cpp)
      reset_rate = true;
      h = std::max(dtmin * 10, std::min(h, tb_code / 10.0));
    }
    if (hit_bp && t < t1 && tb_jump()) {
      nhist = 1; k = 1; steps_at_order = 0; reset_rate = true;
      double nb = t1;
      for (size_t b = ibp; b < bps.size(); ++b) if (bps[b] > t * (1 + 1e-15)) { nb = bps[b]; break; }
      h = first_step(h, t, nb, dtmin);
    }
  }
};

}  // namespace chip
