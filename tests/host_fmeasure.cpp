// Host-only test of the arithmetic of the frequency-domain measurements (cedarsim.jl_amd/csrc/ch_fmeasure_host.hpp): the event rules
// at their edges (g_i == L, a touch without a crossing, n beyond the count, LAST, fd inside an interval), absolute and relative levels,
// LIN and LOG axes, phase wraps in both directions and in two consecutive intervals, windows outside the grid and empty windows, NaN
// rows, |H| = 0, the spec and grid checks, closed-form values and sensitivities, and a serial replay of the wave form (64 chunk scans,
// wrap counts and accumulations combined as fmeasure_wave_kernel combines them) against the one-pass form.  Every expected number is
// worked out by hand in the comments.  Built with sanitizers by tests/test_host_fmeasure.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "ch_fmeasure_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0 || (a != a && b != b); }
static const double INF = std::numeric_limits<double>::infinity(), QNAN = std::numeric_limits<double>::quiet_NaN();
static const double PI = 3.14159265358979323846, LN10 = 2.302585092994045684;

// one sample: rows H[row][nf] as (re, im), sensitivity rows dH[row * n_par + k][nf]
struct Run {
  std::vector<double> f, ulog, H, dH; int n_par = 0;
  void grid(std::vector<double> g) { f = g; ulog.clear(); for (double x : f) ulog.push_back(x > 0 ? std::log10(x) : 0.0); }
  void row(const std::vector<double>& re, const std::vector<double>& im = {}) { for (size_t i = 0; i < re.size(); ++i) { H.push_back(re[i]); H.push_back(im.empty() ? 0.0 : im[i]); } }
  void drow(const std::vector<double>& re, const std::vector<double>& im = {}) { for (size_t i = 0; i < re.size(); ++i) { dH.push_back(re[i]); dH.push_back(im.empty() ? 0.0 : im[i]); } }
  void polar(const std::vector<double>& deg, double mag = 1.0) { for (double d : deg) { H.push_back(mag * std::cos(d * PI / 180)); H.push_back(mag * std::sin(d * PI / 180)); } }
  FRows rows() const {
    FRows R; R.f = f.data(); R.ulog = ulog.data(); R.nf = (long)f.size();
    R.H = H.data(); R.ldH = 1; R.dH = dH.empty() ? nullptr : dH.data(); R.ldS = 1; R.n_par = n_par;
    return R;
  }
};
static ch_fmeasure_side side(int a, int sig = CH_FSIG_RE, double level = 0.0, int edge = CH_EDGE_RISE, int count = 1, double fd = -INF, double ref_at = QNAN, int b = -1,
                             double scale = 1.0) {
  ch_fmeasure_side s; s.row_a = a; s.row_b = b; s.scale = scale; s.sig = sig; s.edge = edge; s.level = level; s.ref_at = ref_at; s.count = count; s.reserved = 0; s.fd = fd; return s;
}
static ch_fmeasure_spec spec(int kind, ch_fmeasure_side s1, int xscale = CH_FX_LIN, ch_fmeasure_side s2 = side(0), double at = 1.0, double from = -INF, double to = INF) {
  ch_fmeasure_spec m; m.kind = kind; m.xscale = xscale; m.s1 = s1; m.s2 = s2; m.at = at; m.from = from; m.to = to; return m;
}
static ch_fmeasure_spec window(int kind, ch_fmeasure_side s1, double from, double to, int xscale = CH_FX_LIN) { return spec(kind, s1, xscale, side(0), 1.0, from, to); }
struct Out { double v; int st; double d[4]; };
static Out eval(const Run& r, const ch_fmeasure_spec& sp) {
  Out o; o.v = 0; for (double& x : o.d) x = 0;
  o.st = fmeas_eval(r.rows(), sp, 0, &o.v, r.n_par ? o.d : nullptr, 1);
  return o;
}

// ---- the wave form replayed serially: 64 lanes' records combined in fmeasure_wave_kernel's order ----
struct Lanes { long ia[64], ib[64], k0[64]; };
static Lanes lanes_of(const FRows& R, const FSig& y) {
  Lanes L; long run = 0;
  for (int l = 0; l < 64; ++l) { meas_lane_chunk(R.nf, l, L.ia[l], L.ib[l]); L.k0[l] = run; run += y.kcount(L.ia[l], L.ib[l]); }   // exclusive prefix sum
  return L;
}
static long wave_k_at(const FSig& y, const Lanes& L, long row) {
  if (y.sig != CH_FSIG_PHASE) return 0;
  long k = 0;
  for (int l = 0; l < 64; ++l) k += y.kcount(L.ia[l], L.ib[l] < row + 1 ? L.ib[l] : row + 1);
  return k;
}
static FFound wave_search(const FRows& R, int xs, const FSig& y, const ch_fmeasure_side& sd, double Lv, const Lanes& L) {
  FScan sc[64]; long first_nf = R.nf, excl = 0, found = -1, kf = 0;
  for (int l = 0; l < 64; ++l) { sc[l] = fmeas_scan(R, xs, y, sd, Lv, L.ia[l], L.ib[l], L.k0[l], 0); if (sc[l].first_nf < first_nf) first_nf = sc[l].first_nf; }
  if (R.nf == 1 && !meas_finite(y.raw(0))) first_nf = 0;
  for (int l = 0; l < 64; ++l) {
    if (sd.count > 0) { if (excl < sd.count && sd.count <= excl + sc[l].count) { const FScan h = fmeas_scan(R, xs, y, sd, Lv, L.ia[l], L.ib[l], L.k0[l], sd.count - excl); found = h.hit; kf = h.khit; } }
    else if (sc[l].last > found) { found = sc[l].last; kf = sc[l].klast; }
    excl += sc[l].count;
  }
  return fmeas_found(sd, found, found >= 0 ? kf : 0, first_nf, R.nf);
}
static Out wave_eval(const Run& r, const ch_fmeasure_spec& sp) {
  const FRows R = r.rows();
  Out o; o.v = 0; for (double& x : o.d) x = 0;
  double* sens = r.n_par ? o.d : nullptr;
  const FSig y = fmeas_signal(R, sp.s1, 0);
  const Lanes L = lanes_of(R, y);
  if (sp.kind == CH_FMEAS_FIND_AT) { FAt p; fmeas_find_at_locate(R, sp, p); o.st = fmeas_find_at(R, sp, 0, p, wave_k_at(y, L, p.upper()), &o.v, sens, 1); return o; }
  if (fmeas_is_event_kind(sp.kind)) {
    FLevel lv; fmeas_level_locate(R, sp.xscale, sp.s1, lv);
    fmeas_level_value(y, sp.s1, lv.rel ? wave_k_at(y, L, lv.p.upper()) : 0, lv);
    const FFound f = wave_search(R, sp.xscale, y, sp.s1, lv.L, L);
    const FSig y2 = fmeas_signal(R, sp.s2, 0);
    const long k2 = (sp.kind == CH_FMEAS_FIND_WHEN && f.i >= 0) ? wave_k_at(y2, lanes_of(R, y2), f.i) : 0;
    o.st = fmeas_finish_event(R, sp, 0, lv, f, k2, &o.v, sens, 1);
    return o;
  }
  double from, to; fmeas_clip(R, sp, from, to);
  auto combined = [&](const FSig* sn) {
    MeasAcc a[64];
    for (int l = 0; l < 64; ++l) { a[l].clear(); fmeas_window_chunk(R, sp.xscale, y, sn, from, to, L.ia[l], L.ib[l], L.k0[l], a[l]); }
    for (int d = 1; d < 64; d <<= 1) for (int l = 0; l < 64; l += 2 * d) a[l].add(a[l + d]);
    return a[0];
  };
  o.st = meas_window_value(fmeas_window_kind(sp.kind), combined(nullptr), from, to, &o.v);
  for (int k = 0; k < r.n_par; ++k) {
    if (o.st != MEAS_OK) { o.d[k] = QNAN; continue; }
    const FSig sn = fmeas_sens_signal(R, sp.s1, 0, k);
    o.d[k] = fmeas_window_sens(sp.kind, R, sp.xscale, y, sn, combined(&sn), from, to);
  }
  return o;
}

static void test_event_rules() {
  Run r; r.grid({1, 2, 3, 4, 5}); r.row({0, 1, 1, 0, 2});
  // rise against 1: 0 < 1 <= 1 in interval 1, g_1 == L: the event is f_1 = 2 exactly
  Out o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0, CH_EDGE_RISE)));
  CHECK(o.st == 0 && o.v == 2.0);
  // the second rise: 0 < 1 <= 2 in interval 4, at 4 + 0.5
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0, CH_EDGE_RISE, 2)));
  CHECK(o.st == 0 && o.v == 4.5);
  // fall against 1: interval 2 is 1 -> 1 (a touch, no event), interval 3 is 1 -> 0: g_2 > 1 is false; no fall at all
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0, CH_EDGE_FALL)));
  CHECK(o.st == MEAS_NOT_FOUND && o.v != o.v);
  // fall against 0.5: interval 3, 1 -> 0, at 3.5; cross counts rise (1.5), fall (3.5), rise (4.25): the third and the last
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5, CH_EDGE_FALL)));
  CHECK(o.st == 0 && o.v == 3.5);
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5, CH_EDGE_CROSS, 3)));
  CHECK(o.st == 0 && o.v == 4.25);
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5, CH_EDGE_CROSS, CH_MEAS_LAST)));
  CHECK(o.st == 0 && o.v == 4.25);
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5, CH_EDGE_CROSS, 4)));
  CHECK(o.st == MEAS_NOT_FOUND);
  // fd = 1.6 sits inside interval 1 behind its event (1.5): the first counted cross is the fall at 3.5; fd = 1.5 still counts it
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5, CH_EDGE_CROSS, 1, 1.6)));
  CHECK(o.st == 0 && o.v == 3.5);
  o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5, CH_EDGE_CROSS, 1, 1.5)));
  CHECK(o.st == 0 && o.v == 1.5);
  // a touch from below: 0 -> 1 -> 0 against 1 is a rise (g_1 == L) and no fall
  Run t; t.grid({1, 2, 3}); t.row({0, 1, 0});
  CHECK(eval(t, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0, CH_EDGE_CROSS, 2))).st == MEAS_NOT_FOUND);
  CHECK(eval(t, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0, CH_EDGE_CROSS, 1))).v == 2.0);
  // one row: nothing to find, FIND_AT reads it, a window is empty
  Run one; one.grid({7}); one.row({3});
  CHECK(eval(one, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0))).st == MEAS_NOT_FOUND);
  CHECK(eval(one, spec(CH_FMEAS_FIND_AT, side(0), CH_FX_LIN, side(0), 9.0)).v == 3.0);
  CHECK(eval(one, window(CH_FMEAS_INTEG, side(0), -INF, INF)).st == MEAS_EMPTY);
}

static void test_interpolation_and_sens() {
  // LIN: rows (1, 0), (3, 2), level 0.5: f* = 1 + 0.25 * 2 = 1.5; weights 0.75, 0.25
  Run r; r.grid({1, 3, 4}); r.row({0, 2, 2}); r.row({10, 20, 40}); r.n_par = 1; r.drow({1, 3, 0}); r.drow({1, 2, 0});
  Out o = eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5)));
  // g_s(u*) = 0.75 * 1 + 0.25 * 3 = 1.5, g' = 1: du*/dp = (0 - 1.5) / 1
  CHECK(o.st == 0 && o.v == 1.5 && o.d[0] == -1.5);
  // FIND_WHEN row 1 there: 0.75 * 10 + 0.25 * 20 = 12.5; g2_s = 0.75 + 0.5 = 1.25, g2' = 5: 1.25 + 5 * (-1.5) = -6.25
  o = eval(r, spec(CH_FMEAS_FIND_WHEN, side(0, CH_FSIG_RE, 0.5), CH_FX_LIN, side(1)));
  CHECK(o.st == 0 && o.v == 12.5 && o.d[0] == -6.25);
  // FIND_AT 3.5 of row 1: 30; sens 0.5 * 2 + 0.5 * 0 = 1; below and above the grid: the end rows
  o = eval(r, spec(CH_FMEAS_FIND_AT, side(1), CH_FX_LIN, side(0), 3.5));
  CHECK(o.st == 0 && o.v == 30.0 && o.d[0] == 1.0);
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(1), CH_FX_LIN, side(0), 0.5)).v == 10.0);
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(1), CH_FX_LIN, side(0), 50.0)).v == 40.0);
  // a row difference and a scale: 2 * (row1 - row0) at 1 is 20
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(1, CH_FSIG_RE, 0, CH_EDGE_RISE, 1, -INF, QNAN, 0, 2.0), CH_FX_LIN, side(0), 1.0)).v == 20.0);
  // relative level: rows 4, 2, 0 at 1, 2, 3; level -1 below g(1) = 4 is 3: the fall in interval 1 at 1.5.  With dre = (1, 0, 0):
  // dL/dp = 1, g_s(u*) = 0.5, g' = -2: du*/dp = (1 - 0.5) / -2 = -0.25 (dropping dL/dp gives +0.25)
  Run q; q.grid({1, 2, 3}); q.row({4, 2, 0}); q.n_par = 1; q.drow({1, 0, 0});
  o = eval(q, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, -1.0, CH_EDGE_FALL, 1, -INF, 1.0)));
  CHECK(o.st == 0 && o.v == 1.5 && o.d[0] == -0.25);
  // the reference inside an interval: g(1.5) = 3, level -2: L = 1, the fall in interval 2 at 2.5; dL/dp = 0.5, g_s = 0: du = 0.5 / -2
  o = eval(q, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, -2.0, CH_EDGE_FALL, 1, -INF, 1.5)));
  CHECK(o.st == 0 && o.v == 2.5 && o.d[0] == -0.25);
  // LOG: f = 1, 10, 100, rows 0, 1, 2, level 0.5: u* = 0.5, f* = sqrt(10); dre = 1: du = -1, df = -ln 10 f*
  Run l; l.grid({1, 10, 100}); l.row({0, 1, 2}); l.n_par = 1; l.drow({1, 1, 1});
  o = eval(l, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.5), CH_FX_LOG));
  CHECK(o.st == 0 && near(o.v, std::sqrt(10.0), 1e-14) && near(o.d[0], -LN10 * std::sqrt(10.0), 1e-13));
  // g_i == L on a LOG axis is f_i itself, not 10^log10(f_i)
  o = eval(l, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 1.0), CH_FX_LOG));
  CHECK(o.st == 0 && o.v == 10.0);
  // signals and their derivatives at H = 3 + 4j, dH = 1 + 2j: |H| = 5; Re(conj H dH) = 11, Im(conj H dH) = 2
  Run s; s.grid({1, 2}); s.row({3, 3}, {4, 4}); s.n_par = 1; s.drow({1, 1}, {2, 2});
  o = eval(s, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_MAG)));
  CHECK(o.v == 5.0 && near(o.d[0], 11.0 / 5.0, 1e-15));
  o = eval(s, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_DB)));
  CHECK(near(o.v, 20.0 * std::log10(5.0), 1e-14) && near(o.d[0], 20.0 / LN10 * 11.0 / 25.0, 1e-15));
  o = eval(s, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE)));
  CHECK(near(o.v, std::atan2(4.0, 3.0) * 180 / PI, 1e-13) && near(o.d[0], 180.0 / PI * 2.0 / 25.0, 1e-15));
  o = eval(s, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_IM)));
  CHECK(o.v == 4.0 && o.d[0] == 2.0);
  o = eval(s, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_DB10)));
  CHECK(near(o.v, 10.0 * std::log10(3.0), 1e-14) && near(o.d[0], 10.0 / LN10 / 3.0, 1e-15));
}

static void test_phase_wraps() {
  // the phase falls through -180: raw 170 -> -170 is an increment of -340 (<= -180): k = +1, 190; then 210
  Run a; a.grid({1, 2, 3}); a.polar({170, -170, -150});
  CHECK(near(eval(a, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 2.0)).v, 190.0, 1e-9));
  CHECK(near(eval(a, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 3.0)).v, 210.0, 1e-9));
  // between rows the line runs through the unwrapped values: at 1.5, 180
  CHECK(near(eval(a, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 1.5)).v, 180.0, 1e-9));
  // the other direction: -170 -> 170 is +340 (> 180): k = -1, -190; then -210; the crossing of -180 is a fall at 1.5
  Run b; b.grid({1, 2, 3}); b.polar({-170, 170, 150});
  CHECK(near(eval(b, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 3.0)).v, -210.0, 1e-9));
  Out o = eval(b, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_PHASE, -180.0, CH_EDGE_FALL)));
  CHECK(o.st == 0 && near(o.v, 1.5, 1e-9));
  // wraps in two consecutive intervals: 170, -170, 170 is 170, 190, 170 (k = 0, 1, 0); then a third: -170 again is 190
  Run c; c.grid({1, 2, 3, 4}); c.polar({170, -170, 170, -170});
  CHECK(near(eval(c, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 3.0)).v, 170.0, 1e-9));
  CHECK(near(eval(c, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 4.0)).v, 190.0, 1e-9));
  CHECK(near(eval(c, window(CH_FMEAS_MAX, side(0, CH_FSIG_PHASE), -INF, INF)).v, 190.0, 1e-9));
  CHECK(near(eval(c, window(CH_FMEAS_INTEG, side(0, CH_FSIG_PHASE), -INF, INF)).v, 3 * 180.0, 1e-9));
  // three poles' worth of phase, 0 -> -270 in steps of 45: the unwrapped phase passes -180 at row 4 (g_4 == L up to rounding)
  Run d; d.grid({1, 2, 3, 4, 5, 6, 7}); d.polar({0, -45, -90, -135, 180, 135, 90}); d.row({0, 1, 2, 3, 4, 5, 6});
  CHECK(near(eval(d, spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), CH_FX_LIN, side(0), 7.0)).v, -270.0, 1e-9));
  o = eval(d, spec(CH_FMEAS_FIND_WHEN, side(0, CH_FSIG_PHASE, -200.0, CH_EDGE_FALL), CH_FX_LIN, side(1)));
  CHECK(o.st == 0 && near(o.v, 4.0 + 20.0 / 45.0, 1e-9));   // between rows 4 (-180) and 5 (-225)
  // FIND_WHEN reads a PHASE as the second signal with its own wrap count: row 1 (index 1 of the run) at the event of row 1's RE
  o = eval(d, spec(CH_FMEAS_FIND_WHEN, side(1, CH_FSIG_RE, 5.5), CH_FX_LIN, side(0, CH_FSIG_PHASE)));
  CHECK(o.st == 0 && near(o.v, -247.5, 1e-9));
}

static void test_windows() {
  Run r; r.grid({0, 1, 2}); r.row({1, 3, 2}); r.n_par = 1; r.drow({1, 2, 4});
  // [0.5, 1.5]: g = 2, 3, 2.5: 0.5 * (2 + 3) * 0.5 + 0.5 * (3 + 2.5) * 0.5 = 2.625; s = 1.5, 2, 3: 0.875 + 1.25 = 2.125
  Out o = eval(r, window(CH_FMEAS_INTEG, side(0), 0.5, 1.5));
  CHECK(o.st == 0 && o.v == 2.625 && o.d[0] == 2.125);
  o = eval(r, window(CH_FMEAS_AVG, side(0), 0.5, 1.5));
  CHECK(o.v == 2.625 && o.d[0] == 2.125);
  // extrema over the point set {from, row 1, to}: max 3 at row 1 (sens 2), min 2 at from (sens 1.5), pp 1 (0.5)
  o = eval(r, window(CH_FMEAS_MAX, side(0), 0.5, 1.5)); CHECK(o.v == 3.0 && o.d[0] == 2.0);
  o = eval(r, window(CH_FMEAS_MIN, side(0), 0.5, 1.5)); CHECK(o.v == 2.0 && o.d[0] == 1.5);
  o = eval(r, window(CH_FMEAS_PP, side(0), 0.5, 1.5)); CHECK(o.v == 1.0 && o.d[0] == 0.5);
  // a window wider than the grid is the grid: 2 + 2.5; an end on a row is that row: [1, 2] max 3 at the from point, sens 2
  o = eval(r, window(CH_FMEAS_INTEG, side(0), -5.0, 10.0)); CHECK(o.st == 0 && o.v == 4.5);
  o = eval(r, window(CH_FMEAS_MAX, side(0), 1.0, 2.0)); CHECK(o.v == 3.0 && o.d[0] == 2.0);
  o = eval(r, window(CH_FMEAS_MIN, side(0), 0.0, 1.5)); CHECK(o.v == 1.0 && o.d[0] == 1.0);
  // ties: first occurrence.  rows 2, 2: min at the from point
  Run t; t.grid({0, 1, 2}); t.row({2, 2, 2}); t.n_par = 1; t.drow({1, 2, 3});
  o = eval(t, window(CH_FMEAS_MIN, side(0), -INF, INF)); CHECK(o.v == 2.0 && o.d[0] == 1.0);
  // rms of a constant 2 is 2; d = integ(y s) / (rms span) = (1.5 + 2.5) * 2 / (2 * 2) = 2
  o = eval(t, window(CH_FMEAS_RMS, side(0), -INF, INF)); CHECK(o.v == 2.0 && o.d[0] == 2.0);
  // empty: from == to, a window beyond the grid, to < from
  CHECK(eval(r, window(CH_FMEAS_INTEG, side(0), 1.0, 1.0)).st == MEAS_EMPTY);
  CHECK(eval(r, window(CH_FMEAS_MAX, side(0), 5.0, 6.0)).st == MEAS_EMPTY);
  CHECK(eval(r, window(CH_FMEAS_AVG, side(0), 1.5, 0.5)).st == MEAS_EMPTY);
  // LOG axis: the ends are read on the line in log10 f, the trapezoids are in f.  rows 0, 1, 2 at 1, 10, 100; [sqrt 10, 10]: g = 0.5, 1
  Run l; l.grid({1, 10, 100}); l.row({0, 1, 2});
  o = eval(l, window(CH_FMEAS_INTEG, side(0), std::sqrt(10.0), 10.0, CH_FX_LOG));
  CHECK(near(o.v, 0.75 * (10.0 - std::sqrt(10.0)), 1e-13));
  // an integrated PSD through DB10: rows 10, 100 are 10, 20 dB
  Run p; p.grid({1, 2}); p.row({10, 100});
  CHECK(near(eval(p, window(CH_FMEAS_AVG, side(0, CH_FSIG_DB10), -INF, INF)).v, 15.0, 1e-13));
}

static void test_nonfinite() {
  Run r; r.grid({1, 2, 3, 4}); r.row({0, QNAN, 2, 3}); r.row({0, 1, 2, 3}); r.row({1, 0, 1, 1}, {0, 0, 0, 0});
  CHECK(eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 2.5))).st == MEAS_NONFINITE);     // the event in interval 3 is behind the NaN row
  CHECK(eval(r, spec(CH_FMEAS_WHEN, side(1, CH_FSIG_RE, 0.5))).st == MEAS_OK);
  CHECK(eval(r, spec(CH_FMEAS_FIND_WHEN, side(1, CH_FSIG_RE, 1.5), CH_FX_LIN, side(0))).st == MEAS_NONFINITE);   // s2 reads rows 1, 2
  CHECK(eval(r, spec(CH_FMEAS_FIND_WHEN, side(1, CH_FSIG_RE, 2.5), CH_FX_LIN, side(0))).st == MEAS_OK);           // rows 2, 3
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(0), CH_FX_LIN, side(0), 1.5)).st == MEAS_NONFINITE);
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(0), CH_FX_LIN, side(0), 3.5)).st == MEAS_OK);
  CHECK(eval(r, window(CH_FMEAS_INTEG, side(0), -INF, INF)).st == MEAS_NONFINITE);
  CHECK(eval(r, window(CH_FMEAS_INTEG, side(0), 3.0, 4.0)).st == MEAS_OK);
  // |H| = 0 at row 1 of row 2: DB and PHASE are not finite there, MAG is 0
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(2, CH_FSIG_DB), CH_FX_LIN, side(0), 2.0)).st == MEAS_NONFINITE);
  CHECK(eval(r, spec(CH_FMEAS_FIND_AT, side(2, CH_FSIG_PHASE), CH_FX_LIN, side(0), 2.0)).st == MEAS_NONFINITE);
  CHECK(eval(r, window(CH_FMEAS_MIN, side(2, CH_FSIG_PHASE), -INF, INF)).st == MEAS_NONFINITE);
  Out o = eval(r, spec(CH_FMEAS_FIND_AT, side(2, CH_FSIG_MAG), CH_FX_LIN, side(0), 2.0));
  CHECK(o.st == MEAS_OK && o.v == 0.0);
  // a relative level whose reference is not finite
  CHECK(eval(r, spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.0, CH_EDGE_RISE, 1, -INF, 2.0))).st == MEAS_NONFINITE);
}

static void test_checks() {
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0)), 1) == nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(1)), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_N_KINDS, side(0)), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0), 2), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_N)), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.0, CH_EDGE_RISE, 0)), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, QNAN)), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.0, 4)), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_RE, 0.0, CH_EDGE_RISE, 1, -INF, -1.0), CH_FX_LOG), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_FIND_WHEN, side(0), CH_FX_LIN, side(3)), 2) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_FIND_AT, side(0), CH_FX_LOG, side(0), 0.0), 1) != nullptr);
  CHECK(fmeas_spec_check(spec(CH_FMEAS_FIND_AT, side(0), CH_FX_LIN, side(0), QNAN), 1) != nullptr);
  CHECK(fmeas_spec_check(window(CH_FMEAS_RMS, side(0), QNAN, 1.0), 1) != nullptr);
  const double ok[3] = {0.0, 1.0, 2.0}, flat[3] = {1.0, 1.0, 2.0}, inf[2] = {1.0, INF};
  CHECK(fmeas_grid_check(ok, 3, false) == nullptr && fmeas_grid_check(ok, 3, true) != nullptr);
  CHECK(fmeas_grid_check(flat, 3, false) != nullptr && fmeas_grid_check(inf, 2, false) != nullptr);
}

// the 64-chunk form against the one-pass form on grids around the chunk sizes, with a phase that wraps every few rows
static void test_wave_replay() {
  const int sizes[] = {1, 2, 3, 63, 64, 65, 129, 200};
  for (int nf : sizes) {
    Run r; std::vector<double> f, deg, re, d0, d1;
    for (int i = 0; i < nf; ++i) {
      f.push_back(10.0 * std::pow(10.0, 4.0 * i / (nf > 1 ? nf - 1 : 1)));
      deg.push_back(std::fmod(20.0 - 97.0 * i + 180.0, 360.0) - 180.0 + (i % 7 == 3 ? 150.0 * ((i / 7) % 2 ? 1 : -1) : 0.0));
      re.push_back(std::sin(0.37 * i) + 0.01 * i); d0.push_back(std::cos(0.2 * i)); d1.push_back(0.5 + 0.1 * i);
    }
    r.grid(f); r.polar(deg, 2.0); r.row(re); r.n_par = 2;
    r.drow(d0, d1); r.drow(d1, d0); r.drow(d1); r.drow(d0);
    const double mid = f[nf / 2] * 1.1, lo = f[0] * 1.3, hi = f[nf - 1] * 0.7;
    std::vector<ch_fmeasure_spec> exact, sums;
    for (int xs : {CH_FX_LIN, CH_FX_LOG}) {
      for (int cnt : {1, 2, 5, 40, CH_MEAS_LAST}) {
        exact.push_back(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_PHASE, -1000.0, CH_EDGE_FALL, cnt), xs));
        exact.push_back(spec(CH_FMEAS_WHEN, side(1, CH_FSIG_RE, 0.3, CH_EDGE_CROSS, cnt, lo), xs));
        exact.push_back(spec(CH_FMEAS_FIND_WHEN, side(1, CH_FSIG_RE, 0.3, CH_EDGE_RISE, cnt), xs, side(0, CH_FSIG_PHASE)));
        exact.push_back(spec(CH_FMEAS_WHEN, side(0, CH_FSIG_PHASE, -500.0, CH_EDGE_CROSS, cnt, -INF, mid), xs));
      }
      exact.push_back(spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), xs, side(0), mid));
      exact.push_back(spec(CH_FMEAS_FIND_AT, side(0, CH_FSIG_PHASE), xs, side(0), f[nf - 1]));
      for (int kind : {CH_FMEAS_MIN, CH_FMEAS_MAX, CH_FMEAS_PP}) { exact.push_back(window(kind, side(0, CH_FSIG_PHASE), lo, hi, xs)); exact.push_back(window(kind, side(1), -INF, INF, xs)); }
      for (int kind : {CH_FMEAS_INTEG, CH_FMEAS_AVG, CH_FMEAS_RMS}) { sums.push_back(window(kind, side(0, CH_FSIG_PHASE), lo, hi, xs)); sums.push_back(window(kind, side(1), -INF, INF, xs)); }
    }
    for (const ch_fmeasure_spec& sp : exact) {
      const Out a = eval(r, sp), b = wave_eval(r, sp);
      CHECK(a.st == b.st && same(a.v, b.v) && same(a.d[0], b.d[0]) && same(a.d[1], b.d[1]));
    }
    for (const ch_fmeasure_spec& sp : sums) {
      const Out a = eval(r, sp), b = wave_eval(r, sp);
      const double tol = 1e-12 * (1.0 + std::fabs(a.v));
      CHECK(a.st == b.st && (a.st != 0 || (near(a.v, b.v, tol) && near(a.d[0], b.d[0], 1e-12 * (1.0 + std::fabs(a.d[0]))) && near(a.d[1], b.d[1], 1e-12 * (1.0 + std::fabs(a.d[1]))))));
    }
  }
}

int main() {
  test_event_rules();
  test_interpolation_and_sens();
  test_phase_wraps();
  test_windows();
  test_nonfinite();
  test_checks();
  test_wave_replay();
  std::printf("fmeasure host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
