// Host-side time stepping (ch_stepper_host.hpp) under AddressSanitizer / UBSan: properties of the source break points, of the
// source values around them, of the BDF / extrapolation weights and of the step controller.  No recorded numbers: every check is
// a property that follows from the definitions.  One more case holds the launch statistics (LaunchStats) to the formulae they
// replaced, on a few counter sets.  Prints "stepper fuzz ok" and returns 0 when all hold.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "ch_stepper_host.hpp"

using namespace chip;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_fail <= 20) { std::printf("FAIL %s:%d %s : ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static std::mt19937_64 rng(20261);
static double uni(double a, double b) { return a + (b - a) * std::uniform_real_distribution<double>(0.0, 1.0)(rng); }
static int irand(int a, int b) { return (int)(a + rng() % (uint64_t)(b - a + 1)); }

// A random source whose segments are no shorter than 1e-3*T (finite slopes: a value changes by far less than 1e-9 of the
// amplitude across one ulp of time) and whose PULSE fits inside its period (no jump where `t mod period` wraps).
// Zero rise / fall times (vertical edges) are given to one-shot pulses only: an edge of a periodic pulse sits at td + k*period, a
// rounded number, and `t mod period` there lands an ulp on either side of the edge — whether source_jumps_at (left limit against
// the value AT t) sees the jump is then decided by that rounding, in the engine and in the oracle alike, so no property of the
// definitions holds for such an edge (it is coded as a corner of length 0 when the rounding hides it; the first step behind it is
// 10*dtmin and the controller steps across).  PWL tables and one-shot pulses, whose edge times are exact, cover vertical edges.
static HSource random_source(double T) {
  HSource s; s.dc = 0.0;
  for (double& p : s.par) p = 0.0;
  const int kinds[3] = {CH_SRC_PWL, CH_SRC_PULSE, CH_SRC_SIN};
  s.kind = kinds[irand(0, 2)];
  if (s.kind == CH_SRC_PWL) {
    const int n = irand(2, 12);
    double t = uni(0.0, 0.1) * T, y = uni(-2.0, 2.0);
    for (int i = 0; i < n; ++i) {
      s.ts.push_back(t); s.ys.push_back(y);
      if (irand(0, 4) == 0 && i + 1 < n) { y += (irand(0, 1) ? 1.0 : -1.0) * uni(0.5, 2.0); s.ts.push_back(t); s.ys.push_back(y); ++i; }   // vertical edge: the value jumps
      t += uni(1e-3, 0.2) * T;
      if (irand(0, 3) != 0) y = uni(-2.0, 2.0);   // else a flat segment
    }
  } else if (s.kind == CH_SRC_PULSE) {
    const double per = uni(0.05, 0.6) * T;
    s.par[0] = uni(-1.0, 1.0); s.par[1] = s.par[0] + (irand(0, 1) ? 1.0 : -1.0) * uni(0.5, 3.0);
    s.par[2] = uni(0.01, 0.1) * per;                              // delay
    s.par[6] = irand(0, 2) == 0 ? INFINITY : per;
    const bool one_shot = !std::isfinite(s.par[6]);
    s.par[3] = (one_shot && irand(0, 1)) ? 0.0 : uni(0.02, 0.2) * per;     // rise (0: a jump)
    s.par[4] = (one_shot && irand(0, 1)) ? 0.0 : uni(0.02, 0.2) * per;     // fall
    s.par[5] = uni(0.1, 0.3) * per;                                        // width
  } else {
    const double f = uni(1.0, 20.0) / T;
    s.par[0] = uni(-1.0, 1.0); s.par[1] = uni(0.1, 2.0); s.par[2] = f; s.par[3] = uni(0.0, 0.2) * T; s.par[4] = uni(0.0, 3.0) / T;
    s.par[5] = irand(0, 1) ? 0.0 : uni(-180.0, 180.0); s.par[6] = irand(0, 1) ? 1e30 : (double)irand(2, 12);
  }
  return s;
}
static double amplitude(const HSource& s) {   // the scale source_jumps_at measures a jump against
  double amp = 0.0;
  if (s.kind == CH_SRC_PWL) for (double y : s.ys) amp = std::max(amp, std::fabs(y));
  else if (s.kind == CH_SRC_PULSE) amp = std::max(std::fabs(s.par[0]), std::fabs(s.par[1]));
  else amp = std::fabs(s.par[0]) + std::fabs(s.par[1]);
  return amp;
}

static void make_breakpoints(const std::vector<HSource>& src, double t0, double t1, std::vector<double>& bps, std::vector<double>& bpc) {
  std::vector<std::pair<double, double>> pts;
  for (const HSource& s : src) source_breakpoint_codes(s, s.par, t0, t1, pts);
  merge_breakpoints(pts, t1, bps, bpc);
}

static void check_sources(int trials) {
  for (int trial = 0; trial < trials; ++trial) {
    const double T = std::pow(10.0, uni(-9.0, 0.0)), t0 = irand(0, 1) ? 0.0 : uni(0.0, 0.3) * T, t1 = t0 + uni(0.3, 1.5) * T;
    std::vector<HSource> src;
    for (int i = irand(1, 4); i > 0; --i) src.push_back(random_source(T));
    std::vector<double> bps, bpc;
    make_breakpoints(src, t0, t1, bps, bpc);
    CHECK(!bps.empty() && bps.size() == bpc.size(), "sizes %zu %zu", bps.size(), bpc.size());
    if (bps.empty()) continue;
    CHECK(bps.back() == t1 && bpc.back() == -1.0, "the list ends at t1 with code -1: %.17g %.17g code %g", bps.back(), t1, bpc.back());
    for (size_t i = 0; i < bps.size(); ++i) {
      CHECK(bps[i] > t0 && bps[i] <= t1, "break point outside (t0, t1]: %.17g", bps[i]);
      if (i > 0) CHECK(bps[i] > bps[i - 1], "not strictly increasing at %zu", i);
    }
    // expected codes, from each source's own sorted times
    for (size_t i = 0; i + 1 < bps.size(); ++i) {
      bool jump = false; double seg = INFINITY;
      for (const HSource& s : src) {
        if (source_jumps_at(s, s.par, bps[i])) jump = true;
        std::vector<double> own; source_breakpoints(s, s.par, t0, t1, own); std::sort(own.begin(), own.end());
        for (size_t j = 0; j < own.size(); ++j) if (own[j] == bps[i]) seg = std::min(seg, (j + 1 < own.size() ? own[j + 1] : t1) - own[j]);
      }
      if (jump) CHECK(bpc[i] < 0, "a source jumps at %.17g but the code is %g", bps[i], bpc[i]);
      else CHECK(bpc[i] == seg, "corner at %.17g: code %g, shortest segment %g", bps[i], bpc[i], seg);
      if (bpc[i] >= 0) for (const HSource& s : src) {   // continuous there: both one-sided limits agree with the value
        const double v = source_value(s, s.par, 0.0, bps[i], 1), tol = 1e-9 * amplitude(s);
        const double l = source_value(s, s.par, 0.0, std::nextafter(bps[i], -INFINITY), 1), r = source_value(s, s.par, 0.0, std::nextafter(bps[i], INFINITY), 1);
        CHECK(std::fabs(v - l) <= tol && std::fabs(r - v) <= tol, "limits at a corner %.17g: %.17g %.17g %.17g", bps[i], l, v, r);
      }
    }
    for (const HSource& s : src) if (s.kind == CH_SRC_PWL) {
      const size_t n = s.ts.size();
      for (size_t i = 0; i < n; ++i) {
        if ((i > 0 && s.ts[i - 1] == s.ts[i]) || (i + 1 < n && s.ts[i + 1] == s.ts[i])) continue;   // a vertical edge has no single value
        CHECK(source_value(s, s.par, 0.0, s.ts[i], 1) == s.ys[i], "PWL knot %zu: %.17g != %.17g", i, source_value(s, s.par, 0.0, s.ts[i], 1), s.ys[i]);
      }
      CHECK(source_value(s, s.par, 7.5, s.ts[0], 0) == 7.5 && source_value(s, s.par, 0.0, 123.0, 2) == source_value(s, s.par, 0.0, 0.0, 1), "modes 0 (dc) and 2 (t = 0)");
    }
    if (trial % 16 == 0) {   // the A/B switch is read at call time: every break point restarts
      setenv("CEDARHIP_BP_RESTART_ALL", "1", 1);
      std::vector<double> b2, c2; make_breakpoints(src, t0, t1, b2, c2);
      unsetenv("CEDARHIP_BP_RESTART_ALL");
      CHECK(b2 == bps, "the switch must not move break points");
      for (double c : c2) CHECK(c == -1.0, "restart-all code %g", c);
    }
  }
}

// p(x) = ((x - c) / s)^d, one monomial so that its values carry a relative rounding error only
static double mono(double x, double c, double s, int d) { return std::pow((x - c) / s, d); }
static double dmono(double x, double c, double s, int d) { return d == 0 ? 0.0 : d * std::pow((x - c) / s, d - 1) / s; }

static void check_weights(int trials) {
  double worst_e = 0, worst_b = 0;
  for (int trial = 0; trial < trials; ++trial) {
    double tau[9], h = std::pow(10.0, uni(-6.0, 0.0));
    tau[0] = uni(0.0, 1.0);
    // neighbouring step ratios up to 100; steps stay above 1e-9 (times of order 1: far above an ulp) and below 1e3
    for (int j = 1; j < 9; ++j) { tau[j] = tau[j - 1] - h; h = std::min(1e3, std::max(1e-9, h * std::pow(100.0, uni(-1.0, 1.0)))); }
    const double c = tau[irand(0, 8)] + uni(-1.0, 1.0) * (tau[0] - tau[8]), s = tau[0] - tau[8];
    for (int np = 1; np <= 7; ++np) for (int d = 0; d < np; ++d) {
      double w[9] = {0}, sum = 0, mag = 0;
      extrap_weights(tau, np, w);
      for (int j = 1; j <= np; ++j) { const double term = w[j] * mono(tau[j], c, s, d); sum += term; mag += std::fabs(term); }
      const double err = std::fabs(sum - mono(tau[0], c, s, d));
      worst_e = std::max(worst_e, mag > 0 ? err / mag : err);
      CHECK(err <= 1e-12 * mag, "extrap_weights np %d degree %d: error %.3e of %.3e", np, d, err, mag);
    }
    for (int k = 1; k <= 5; ++k) for (int d = 0; d <= k; ++d) {
      double a[9] = {0}, sum = 0, mag = 0;
      bdf_coeffs(tau, k, a);
      for (int j = 0; j <= k; ++j) { const double term = a[j] * mono(tau[j], c, s, d); sum += term; mag += std::fabs(term); }
      const double err = std::fabs(sum - dmono(tau[0], c, s, d));
      worst_b = std::max(worst_b, mag > 0 ? err / mag : err);
      CHECK(err <= 1e-12 * mag, "bdf_coeffs k %d degree %d: error %.3e of %.3e", k, d, err, mag);
    }
  }
  std::printf("weights: worst relative error extrap %.2e, bdf %.2e (bound 1e-12)\n", worst_e, worst_b);
}

static void check_controller(int trials) {
  long n_attempts = 0, n_dtmin = 0, n_done = 0, n_restart = 0;
  for (int trial = 0; trial < trials; ++trial) {
    const double T = std::pow(10.0, uni(-9.0, 0.0)), t0 = 0.0, t1 = uni(0.3, 1.5) * T;
    std::vector<HSource> src;
    for (int i = irand(0, 3); i > 0; --i) src.push_back(random_source(T));
    std::vector<double> bps, bpc;
    make_breakpoints(src, t0, t1, bps, bpc);
    const double span = t1 - t0, dtmin = irand(0, 3) == 0 ? std::pow(10.0, uni(-7.0, -3.0)) * span : 1e-15 * span, dtmax = span / 10.0;
    const int kmax = irand(1, 5);
    const double p_fail = irand(0, 4) == 0 ? 0.6 : 0.08, p_rej = 0.15;
    StepControl sc(t0, t1, irand(0, 1) ? 0.0 : uni(1e-6, 1e-2) * span, dtmin, dtmax, kmax, bps, bpc);
    CHECK(sc.h >= 10 * dtmin && sc.h <= std::max(10 * dtmin, (bps[0] - t0) / 50.0 * FIRST_STEP_FRAC), "first step %.3e", sc.h);
    bool stopped = false;
    for (int attempt = 0; attempt < 200000 && sc.t < t1; ++attempt, ++n_attempts) {
      const double t = sc.t;
      double next_bp = t1; bool next_jump = true;
      for (size_t b = 0; b < bps.size(); ++b) if (bps[b] > t) { next_bp = bps[b]; next_jump = bpc[b] < 0; break; }
      const int rc = sc.plan();
      if (rc != CH_OK) { CHECK(rc == CH_ERR_DTMIN && sc.hh < dtmin, "plan() refused with %d at hh %.3e, dtmin %.3e", rc, sc.hh, dtmin); ++n_dtmin; stopped = true; break; }
      CHECK(sc.hh >= dtmin, "a step of %.3e below dtmin %.3e was planned without CH_ERR_DTMIN", sc.hh, dtmin);
      CHECK(sc.tn > t && sc.tn <= next_bp, "step from %.17g to %.17g past the break point %.17g", t, sc.tn, next_bp);
      CHECK(sc.hit_bp == (sc.tn == next_bp), "hit_bp %d at tn %.17g, break point %.17g", (int)sc.hit_bp, sc.tn, next_bp);
      CHECK(sc.kk >= 1 && sc.kk <= kmax && sc.kk <= sc.nh && sc.c.npred == sc.np && sc.np >= 1 && sc.np <= 7 && sc.c.nkp1 <= 7, "orders: kk %d nh %d np %d nkp1 %d", sc.kk, sc.nh, sc.np, sc.c.nkp1);
      for (int j = 0; j < 7; ++j) CHECK(sc.c.hist_slot[j] >= 0 && sc.c.hist_slot[j] < NSLOT && sc.c.hist_slot[j] != sc.c.cand_slot, "history slot %d", sc.c.hist_slot[j]);
      const double u = uni(0.0, 1.0);
      if (u < p_fail) { sc.on_convergence_failure(); CHECK(sc.k == 1 && sc.nhist <= 2 && sc.nhist >= 1 && sc.reset_rate, "after a convergence failure"); continue; }
      const double errk = sc.lte ? (u < p_fail + p_rej ? uni(1.0, 100.0) + 1e-9 : std::pow(uni(0.0, 1.0), 4)) : 0.0;   // accepted errors mostly small: the step grows
      if (errk > 1.0) { const double hb = sc.h; sc.on_error_test_failure(errk); CHECK(sc.h <= 0.9 * sc.hh && sc.h >= 0.25 * sc.hh * (1 - 1e-15), "reject: h %.3e -> %.3e (attempt %.3e)", hb, sc.h, sc.hh); continue; }
      sc.on_accept();
      { double ww[9]; const int m = sc.dense_weights(0.5 * (t + sc.tn), ww); double sw = 0; for (int j = 1; j <= m; ++j) sw += ww[j];
        CHECK(m == sc.dense_points() && m >= 1 && m <= 7 && std::fabs(sw - 1.0) < 1e-6, "dense output: %d points, weights sum to %.12g", m, sw); }
      sc.select_next(errk, uni(0.0, 2.0), uni(0.0, 2.0));
      CHECK(sc.t == sc.tn && sc.h > 0 && sc.h <= dtmax && sc.k >= 1 && sc.k <= kmax, "after accept: t %.17g h %.3e k %d", sc.t, sc.h, sc.k);
      const bool restarted = sc.nhist == 1;
      CHECK(restarted == (sc.hit_bp && next_jump && sc.t < t1), "restart at order 1 (%d) behind a jump only: hit %d jump %d t %.17g t1 %.17g", (int)restarted, (int)sc.hit_bp, (int)next_jump, sc.t, t1);
      if (restarted) { ++n_restart; CHECK(sc.k == 1 && sc.reset_rate, "restart leaves order %d", sc.k); }
    }
    if (!stopped) { CHECK(sc.t == t1, "the controller ends on t1 exactly: %.17g vs %.17g", sc.t, t1); ++n_done; }
  }
  std::printf("controller: %ld attempts, %ld transients completed, %ld stopped at dtmin, %ld restarts behind jumps\n", n_attempts, n_done, n_dtmin, n_restart);
  CHECK(n_done > 0 && n_dtmin > 0 && n_restart > 0, "the script reaches every outcome");
}

// The launch statistics (LaunchStats) against the formulae the engine used before they were gathered in one place, written out
// here literally: exact equality on hand-picked counter sets, and reset() leaves every field zero.
static void check_launch_stats() {
  struct Set { double device_ms; long n_launch, n_timed; double persist_ms; long persist_launches; double dc_device_ms; long dc_launches, dc_timed; const char* what; };
  const Set sets[] = {
    {0.0, 40, 0, 0.0, 0, 0.0, 7, 0, "no launch timed"},
    {1.7, 123, 17, 0.0, 0, 0.3, 11, 2, "sampled launches, some of them during the initialisation"},
    {0.9, 9, 9, 0.0, 0, 0.9, 9, 9, "every launch timed and all of them initialisation"},
    {0.4, 12, 3, 31.25, 1, 0.4, 12, 3, "a persistent launch behind a sampled operating point"},
    {0.0, 1, 0, 7.5, 3, 0.0, 1, 0, "persistent launches (drained rows), nothing else timed"},
  };
  for (const Set& q : sets) {
    LaunchStats ls;
    ls.device_ms = q.dc_device_ms; ls.n_launch = q.dc_launches; ls.n_timed = q.dc_timed;
    ls.end_of_dc(5);
    ls.device_ms = q.device_ms; ls.n_launch = q.n_launch; ls.n_timed = q.n_timed; ls.persist_ms = q.persist_ms; ls.persist_launches = q.persist_launches;
    ch_stats st; std::memset(&st, 0, sizeof(st));
    ls.fill(st);
    // finish_tran of the parent
    const double device_seconds = (q.n_timed > 0 ? q.device_ms * 1e-3 * (double)q.n_launch / (double)q.n_timed : 0.0) + q.persist_ms * 1e-3;
    double step_kernel_seconds; long step_kernel_launches;
    if (q.persist_launches > 0) { step_kernel_seconds = q.persist_ms * 1e-3; step_kernel_launches = q.persist_launches; }
    else {
      const long nl = q.n_launch - q.dc_launches, ntm = q.n_timed - q.dc_timed;
      step_kernel_launches = nl;
      step_kernel_seconds = ntm > 0 ? (q.device_ms - q.dc_device_ms) * 1e-3 * (double)nl / (double)ntm : 0.0;
    }
    CHECK(st.device_seconds == device_seconds, "%s: device_seconds %.17g vs %.17g", q.what, st.device_seconds, device_seconds);
    CHECK(st.step_kernel_seconds == step_kernel_seconds, "%s: step_kernel_seconds %.17g vs %.17g", q.what, st.step_kernel_seconds, step_kernel_seconds);
    CHECK(st.step_kernel_launches == step_kernel_launches, "%s: step_kernel_launches %ld vs %ld", q.what, (long)st.step_kernel_launches, step_kernel_launches);
    CHECK(ls.dc_block_iters == 5, "%s: end_of_dc keeps the block iterations", q.what);
  }
  {  // an operating point alone (ch_dc of the parent): the sampled launches scaled, no stepping kernels
    LaunchStats ls;
    ls.device_ms = 2.5; ls.n_launch = 14; ls.n_timed = 3;
    ls.end_of_dc(0);
    ch_stats st; std::memset(&st, 0, sizeof(st));
    ls.fill(st);
    const double device_ms = 2.5; const long n_launch = 14, n_timed = 3;
    const double device_seconds = n_timed > 0 ? device_ms * 1e-3 * (double)n_launch / (double)n_timed : 0.0;
    CHECK(st.device_seconds == device_seconds && st.step_kernel_seconds == 0.0 && st.step_kernel_launches == 0, "operating point alone: %.17g vs %.17g, step %.17g / %ld",
          st.device_seconds, device_seconds, st.step_kernel_seconds, (long)st.step_kernel_launches);
    ls.prof_launch = 1; ls.prof_wait = 2; ls.prof_reduce = 3; ls.persist_ms = 4; ls.persist_launches = 5; ls.persist_attempts = 6; ls.persist_barrier_s = 7; ls.dc_block_iters = 8;
    ls.reset();
    CHECK(ls.device_ms == 0 && ls.n_launch == 0 && ls.n_timed == 0 && ls.prof_launch == 0 && ls.prof_wait == 0 && ls.prof_reduce == 0 && ls.persist_ms == 0 &&
          ls.persist_launches == 0 && ls.persist_attempts == 0 && ls.persist_barrier_s == 0 && ls.dc_device_ms == 0 && ls.dc_launches == 0 && ls.dc_timed == 0 &&
          ls.dc_block_iters == 0, "reset() leaves every field zero");
    static_assert(sizeof(LaunchStats) == 7 * sizeof(double) + 5 * sizeof(long) + 2 * sizeof(long long), "a new LaunchStats field belongs in the reset() check above");
  }
}

int main() {
  unsetenv("CEDARHIP_BP_RESTART_ALL");
  check_sources(3000);
  check_weights(20000);
  check_controller(400);
  check_launch_stats();
  CHECK(resolve_stepper(CH_STEPPER_AUTO, nullptr) == CH_STEPPER_AUTO && resolve_stepper(CH_STEPPER_AUTO, "host") == CH_STEPPER_HOST &&
        resolve_stepper(CH_STEPPER_AUTO, "device") == CH_STEPPER_DEVICE && resolve_stepper(CH_STEPPER_AUTO, "device", false) == CH_STEPPER_AUTO &&
        resolve_stepper(CH_STEPPER_DEVICE, "host") == CH_STEPPER_DEVICE && resolve_stepper(CH_STEPPER_AUTO, "other") == CH_STEPPER_AUTO, "resolve_stepper");
  if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }
  std::printf("stepper fuzz ok\n");
  return 0;
}
