// Host-only test of the arithmetic of the waveform measurements (cedarsim.jl_amd/csrc/ch_measure_host.hpp): the event rules at their
// edges (y_i == L, a touch without a crossing, events in the first and in the last interval, a zero-length interval, td behind every
// event and inside an interval, n beyond the count, LAST), m clamped near the start, window ends outside the run and from == to, NaN
// rows, the sample-chunk and lane-chunk rules, closed-form values and sensitivities, and a serial replay of the wave form (64 chunk
// scans and accumulations combined as measure_wave_kernel combines them) against the one-pass form.  Every expected number is worked
// out by hand in the comments.  Built with sanitizers by tests/test_host_measure.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "ch_measure_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }
static const double INF = std::numeric_limits<double>::infinity(), QNAN = std::numeric_limits<double>::quiet_NaN();

// one sample: rows V[row][nt], sensitivity rows Sn[row * n_par + k][nt]
struct Run {
  std::vector<double> t, V, Sn; std::vector<int32_t> pts; int n_par = 0;
  MeasRows rows() const {
    MeasRows R; R.t = t.data(); R.pts = pts.empty() ? nullptr : pts.data(); R.nt = (long)t.size();
    R.V = V.data(); R.ldV = 1; R.Sn = Sn.empty() ? nullptr : Sn.data(); R.ldS = 1; R.n_par = n_par;
    return R;
  }
};
static ch_measure_side side(int a, int b = -1, double scale = 1.0, double level = 0.0, int edge = CH_EDGE_RISE, int count = 1, double td = -INF) {
  ch_measure_side s; s.row_a = a; s.row_b = b; s.scale = scale; s.level = level; s.edge = edge; s.count = count; s.td = td; return s;
}
static ch_measure_spec spec(int kind, ch_measure_side s1, ch_measure_side s2 = side(0), double at = 0.0, double from = -INF, double to = INF) {
  ch_measure_spec m; m.kind = kind; m.reserved = 0; m.s1 = s1; m.s2 = s2; m.at = at; m.from = from; m.to = to; return m;
}
struct Out { double v; int st; double d[4]; };
static Out eval(const Run& r, const ch_measure_spec& sp) {
  Out o; o.v = 0; for (double& x : o.d) x = 0;
  o.st = meas_eval(r.rows(), sp, 0, &o.v, r.n_par ? o.d : nullptr, 1);
  return o;
}
// the wave form replayed serially: 64 lanes' records combined in measure_wave_kernel's order
static MeasFound wave_search(const MeasRows& R, const MeasSig& y, const ch_measure_side& sd) {
  MeasScan sc[64]; long first_nf = R.nt, excl = 0, found = -1;
  for (int l = 0; l < 64; ++l) { long ia, ib; meas_lane_chunk(R.nt, l, ia, ib); sc[l] = meas_scan(R, y, sd, ia, ib, 0); first_nf = std::fmin((double)first_nf, (double)sc[l].first_nf); }
  if (R.nt == 1 && !meas_finite(y.at(0))) first_nf = 0;
  for (int l = 0; l < 64; ++l) {
    long ia, ib; meas_lane_chunk(R.nt, l, ia, ib);
    if (sd.count > 0) { if (excl < sd.count && sd.count <= excl + sc[l].count) found = meas_scan(R, y, sd, ia, ib, sd.count - excl).hit; }
    else if (sc[l].last > found) found = sc[l].last;
    excl += sc[l].count;
  }
  return meas_found(sd, found, first_nf, R.nt);
}
static Out wave_eval(const Run& r, const ch_measure_spec& sp) {
  const MeasRows R = r.rows();
  Out o; o.v = 0; for (double& x : o.d) x = 0;
  double* sens = r.n_par ? o.d : nullptr;
  if (meas_is_event_kind(sp.kind)) {
    const MeasFound f1 = wave_search(R, meas_signal(R, sp.s1, 0), sp.s1);
    MeasFound f2; f2.i = -1; f2.nonfinite = false;
    if (sp.kind == CH_MEAS_DELAY) f2 = wave_search(R, meas_signal(R, sp.s2, 0), sp.s2);
    o.st = meas_finish_event(R, sp, 0, f1, f2, &o.v, sens, 1);
    return o;
  }
  if (sp.kind == CH_MEAS_FIND_AT) { o.st = meas_find_at(R, sp, 0, &o.v, sens, 1); return o; }
  const MeasSig y = meas_signal(R, sp.s1, 0);
  double from, to; meas_clip(R, sp, from, to);
  auto combined = [&](const MeasSig* sn) {
    MeasAcc a[64];
    for (int l = 0; l < 64; ++l) { long ia, ib; meas_lane_chunk(R.nt, l, ia, ib); a[l].clear(); meas_window_chunk(R, y, sn, from, to, ia, ib, a[l]); }
    for (int d = 1; d < 64; d <<= 1) for (int l = 0; l < 64; l += 2 * d) a[l].add(a[l + d]);
    return a[0];
  };
  const MeasAcc a = combined(nullptr);
  o.st = meas_window_value(sp.kind, a, from, to, &o.v);
  for (int k = 0; k < r.n_par; ++k) {
    const MeasSig sn = meas_sens_signal(R, sp.s1, 0, k);
    const MeasAcc ak = combined(&sn);
    o.d[k] = o.st == MEAS_OK ? meas_window_sens(sp.kind, R, sn, ak, from, to) : QNAN;
  }
  return o;
}
static bool same_bits(double a, double b) { return (a != a && b != b) || (a == b && std::signbit(a) == std::signbit(b)); }

// ---- y = p t^2 (row 0) and z = 3 t + 1 (row 1), p = 2, with the run's dense points: the interpolant IS the polynomial from interval 2 on ----
static Run quadratic() {
  Run r; r.t = {0.0, 0.3, 0.5, 0.9, 1.3, 1.4, 2.0}; r.pts = {1, 3, 3, 3, 3, 3, 3}; r.n_par = 1;
  for (double t : r.t) r.V.push_back(2.0 * t * t);
  for (double t : r.t) r.V.push_back(3.0 * t + 1.0);
  for (double t : r.t) r.Sn.push_back(t * t);   // dy/dp
  for (double t : r.t) { (void)t; r.Sn.push_back(0.0); }   // dz/dp
  return r;
}
static void closed_forms() {
  const Run r = quadratic();
  // y = 2.88 at t = 1.2, inside (0.9, 1.3]; dt*/dp = -(t^2) / (2 p t) = -t / (2 p) = -0.3
  Out o = eval(r, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 2.88)));
  CHECK(o.st == MEAS_OK && near(o.v, 1.2, 1e-14) && near(o.d[0], -0.3, 1e-13));
  // the same crossing of -y through -2.88 is a fall; the scale reaches value and sensitivity rows alike
  o = eval(r, spec(CH_MEAS_WHEN, side(0, -1, -1.0, -2.88, CH_EDGE_FALL)));
  CHECK(o.st == MEAS_OK && near(o.v, 1.2, 1e-14) && near(o.d[0], -0.3, 1e-13));
  CHECK(eval(r, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 2.88, CH_EDGE_FALL))).st == MEAS_NOT_FOUND);
  // z at that time: 4.6; d/dp = dz/dp + z' dt*/dp = 0 + 3 (-0.3)
  o = eval(r, spec(CH_MEAS_FIND_WHEN, side(0, -1, 1.0, 2.88), side(1)));
  CHECK(o.st == MEAS_OK && near(o.v, 4.6, 1e-13) && near(o.d[0], -0.9, 1e-12));
  // delay from y = 0.72 (t = 0.6) to z = 5.5 (t = 1.5): 0.9; d/dp = 0 - (-0.6 / 4) = 0.15
  o = eval(r, spec(CH_MEAS_DELAY, side(0, -1, 1.0, 0.72), side(1, -1, 1.0, 5.5)));
  CHECK(o.st == MEAS_OK && near(o.v, 0.9, 1e-13) && near(o.d[0], 0.15, 1e-13));
  // y - z as one signal: 2 t^2 - 3 t - 1 = 1 at t = 2; on the last row exactly (y_i == L): the event time is t_i; d/dp = -4 / (4 p - 3) = -0.8
  o = eval(r, spec(CH_MEAS_WHEN, side(0, 1, 1.0, 1.0)));
  CHECK(o.st == MEAS_OK && o.v == 2.0 && near(o.d[0], -0.8, 1e-12));
  // find-at inside the polynomial's reach: y(1.0) = 2, dy/dp = 1
  o = eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), 1.0));
  CHECK(o.st == MEAS_OK && near(o.v, 2.0, 1e-14) && near(o.d[0], 1.0, 1e-14));
  // m clamped near the start: interval 1 has two rows only, so a line through (0, 0) and (0.3, 0.18): 0.09 at 0.15 (the parabola has 0.045)
  o = eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), 0.15));
  CHECK(o.st == MEAS_OK && near(o.v, 0.09, 1e-15) && near(o.d[0], 0.045, 1e-15));
  // interval 2 already runs through rows 0..2: the parabola itself
  o = eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), 0.4));
  CHECK(o.st == MEAS_OK && near(o.v, 0.32, 1e-15));
  // outside the run: the end rows
  CHECK(eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), -1.0)).v == 0.0 && eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), 7.0)).v == 8.0);
  // window [1.0, 1.35] on y: points (1.0, 2), row 4 (1.3, 3.38), (1.35, 3.645): trapezoid 0.3 * 2.69 + 0.05 * 3.5125 = 0.982625;
  // on dy/dp the same rule over 1, 1.69, 1.8225: half of that
  o = eval(r, spec(CH_MEAS_INTEG, side(0), side(0), 0.0, 1.0, 1.35));
  CHECK(o.st == MEAS_OK && near(o.v, 0.982625, 1e-14) && near(o.d[0], 0.4913125, 1e-14));
  o = eval(r, spec(CH_MEAS_MAX, side(0), side(0), 0.0, 1.0, 1.35));
  CHECK(o.st == MEAS_OK && near(o.v, 3.645, 1e-14) && near(o.d[0], 1.8225, 1e-14));
  o = eval(r, spec(CH_MEAS_PP, side(0), side(0), 0.0, 1.0, 1.35));
  CHECK(o.st == MEAS_OK && near(o.v, 1.645, 1e-14) && near(o.d[0], 0.8225, 1e-14));
}

// ---- piecewise-linear rows (no dense points) with a repeated time: t = 0 1 2 3 4 5 5 6, y = 0 1 1 0 1 2 0.2 0.5; dy/dp = 1 everywhere ----
static Run corners() {
  Run r; r.t = {0, 1, 2, 3, 4, 5, 5, 6}; r.V = {0, 1, 1, 0, 1, 2, 0.2, 0.5}; r.n_par = 1; r.Sn.assign(8, 1.0);
  return r;
}
static void event_rules() {
  const Run r = corners();
  auto when = [&](double L, int edge, int n, double td = -INF) { return eval(r, spec(CH_MEAS_WHEN, side(0, -1, 1.0, L, edge, n, td))); };
  // rises through 1: interval 1 (0 < 1 <= 1, y_i == L: time t_1) and interval 4; the plateau 1 -> 1 and the step 1 -> 2 are none
  CHECK(when(1.0, CH_EDGE_RISE, 1).st == MEAS_OK && when(1.0, CH_EDGE_RISE, 1).v == 1.0);
  CHECK(when(1.0, CH_EDGE_RISE, 2).v == 4.0);
  CHECK(when(1.0, CH_EDGE_RISE, 3).st == MEAS_NOT_FOUND && std::isnan(when(1.0, CH_EDGE_RISE, 3).v) && std::isnan(when(1.0, CH_EDGE_RISE, 3).d[0]));   // n beyond the count
  CHECK(when(1.0, CH_EDGE_RISE, CH_MEAS_LAST).v == 4.0);
  // falls through 1: leaving the plateau (1 > 1 is false) is none; the jump 2 -> 0.2 on the repeated time is one, at t = 5, and does not move
  Out o = when(1.0, CH_EDGE_FALL, 1);
  CHECK(o.st == MEAS_OK && o.v == 5.0 && o.d[0] == 0.0);
  CHECK(when(1.0, CH_EDGE_FALL, 2).st == MEAS_NOT_FOUND);
  // a touch without a crossing: the peak 2 is reached from below (a rise at t = 5) but never left downwards through 2 (2 > 2 is false)
  CHECK(when(2.0, CH_EDGE_RISE, 1).v == 5.0 && when(2.0, CH_EDGE_FALL, 1).st == MEAS_NOT_FOUND);
  CHECK(when(2.5, CH_EDGE_CROSS, CH_MEAS_LAST).st == MEAS_NOT_FOUND);
  // through 0.4: rises in the first interval (0.4), in interval 4 (3.4) and in the last one (0.2 -> 0.5: 5 + 2/3); dt/dp = -1 / slope
  o = when(0.4, CH_EDGE_RISE, 1);
  CHECK(o.st == MEAS_OK && near(o.v, 0.4, 1e-15) && near(o.d[0], -1.0, 1e-14));
  CHECK(near(when(0.4, CH_EDGE_RISE, 2).v, 3.4, 1e-15));
  o = when(0.4, CH_EDGE_RISE, CH_MEAS_LAST);
  CHECK(o.st == MEAS_OK && near(o.v, 5.0 + 2.0 / 3.0, 1e-14) && near(o.d[0], -1.0 / 0.3, 1e-12));
  CHECK(near(when(0.4, CH_EDGE_RISE, 3).v, 5.0 + 2.0 / 3.0, 1e-14));
  // crossings of 0.5 in either direction: 0.5 (rise), 2.5 (fall), 3.5 (rise), 5 (the jump), 6 (y_i == L on the last row)
  CHECK(near(when(0.5, CH_EDGE_CROSS, 2).v, 2.5, 1e-15) && when(0.5, CH_EDGE_CROSS, 4).v == 5.0 && when(0.5, CH_EDGE_CROSS, 5).v == 6.0 && when(0.5, CH_EDGE_CROSS, 6).st == MEAS_NOT_FOUND);
  CHECK(near(when(0.5, CH_EDGE_CROSS, 2).d[0], 1.0, 1e-14));   // falling slope -1: dt/dp = -1 / -1
  // td: inside the first interval before its event (counts), behind it (does not), on a row, behind every event
  CHECK(near(when(0.4, CH_EDGE_RISE, 1, 0.35).v, 0.4, 1e-15) && near(when(0.4, CH_EDGE_RISE, 1, 0.45).v, 3.4, 1e-15));
  CHECK(near(when(0.4, CH_EDGE_RISE, 1, 1.0).v, 3.4, 1e-15) && near(when(0.4, CH_EDGE_RISE, 2, 3.0).v, 5.0 + 2.0 / 3.0, 1e-14));
  CHECK(when(0.4, CH_EDGE_RISE, 1, 5.9).st == MEAS_NOT_FOUND && when(0.4, CH_EDGE_RISE, CH_MEAS_LAST, 5.9).st == MEAS_NOT_FOUND);
  CHECK(when(1.0, CH_EDGE_FALL, 1, 5.0).v == 5.0 && when(1.0, CH_EDGE_FALL, 1, 5.5).st == MEAS_NOT_FOUND);   // the jump sits at t = 5
  // find-when on the jump reads the later row of the repeated time
  o = eval(r, spec(CH_MEAS_FIND_WHEN, side(0, -1, 1.0, 1.0, CH_EDGE_FALL), side(0, -1, 10.0)));
  CHECK(o.st == MEAS_OK && o.v == 2.0 && o.d[0] == 10.0);
  // a single row has no intervals at all
  Run one; one.t = {0.0}; one.V = {1.0};
  CHECK(eval(one, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5))).st == MEAS_NOT_FOUND && eval(one, spec(CH_MEAS_FIND_AT, side(0), side(0), 3.0)).v == 1.0);
  CHECK(eval(one, spec(CH_MEAS_AVG, side(0))).st == MEAS_EMPTY);
  // status 4: rows (0, 0), (1, 0.75), (2, 1) lie on P = 1 - (t - 2)^2 / 4, which reaches 1 at its top: the rise 0.75 < 1 <= 1 of interval 2
  // is an event at t = 2 (y_i == L) with P'(2) = 0: the value stands, the sensitivities are NaN
  Run top; top.t = {0, 1, 2}; top.pts = {1, 2, 3}; top.V = {0, 0.75, 1}; top.n_par = 1; top.Sn = {1, 1, 1};
  o = eval(top, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 1.0)));
  CHECK(o.st == MEAS_FLAT && o.v == 2.0 && std::isnan(o.d[0]));
  top.pts = {1, 2, 2};   // the same rows with a line on interval 2: slope 0.25, dt/dp = -1 / 0.25
  o = eval(top, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 1.0)));
  CHECK(o.st == MEAS_OK && o.v == 2.0 && near(o.d[0], -4.0, 1e-15));
  top.pts = {1, 7, 7};   // dense points beyond i + 1 are clamped: interval 1 is the line of slope 0.75
  o = eval(top, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.375)));
  CHECK(o.st == MEAS_OK && near(o.v, 0.5, 1e-15) && near(o.d[0], -1.0 / 0.75, 1e-15));
  MeasEvent e; e.m = 3; e.dP = 0.0; CHECK(meas_event_flat(e));
  e.dP = 2.0; CHECK(!meas_event_flat(e));
  e.m = 1; e.dP = 0.0; CHECK(!meas_event_flat(e));
}

// ---- windows: y = p t on t = 0 1 2 4 (p = 3, dy/dp = t), and the constant -2 (dy/dp = 1) ----
static void windows() {
  Run r; r.t = {0, 1, 2, 4}; r.V = {0, 3, 6, 12, -2, -2, -2, -2}; r.n_par = 1; r.Sn = {0, 1, 2, 4, 1, 1, 1, 1};
  auto win = [&](int kind, int row, double from, double to) { return eval(r, spec(kind, side(row), side(0), 0.0, from, to)); };
  // [0.5, 3]: integral of 3 t = 1.5 (9 - 0.25) = 13.125, of t: 4.375; the trapezoid rule is exact on a line
  Out o = win(CH_MEAS_INTEG, 0, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && near(o.v, 13.125, 1e-14) && near(o.d[0], 4.375, 1e-14));
  o = win(CH_MEAS_AVG, 0, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && near(o.v, 5.25, 1e-14) && near(o.d[0], 1.75, 1e-14));
  o = win(CH_MEAS_MIN, 0, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && near(o.v, 1.5, 1e-15) && near(o.d[0], 0.5, 1e-15));
  o = win(CH_MEAS_MAX, 0, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && near(o.v, 9.0, 1e-15) && near(o.d[0], 3.0, 1e-15));
  o = win(CH_MEAS_PP, 0, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && near(o.v, 7.5, 1e-15) && near(o.d[0], 2.5, 1e-15));
  // rms of the constant -2 is 2; d/dp = trapz(y s) / (rms T) = -2 T / (2 T)
  o = win(CH_MEAS_RMS, 1, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && near(o.v, 2.0, 1e-15) && near(o.d[0], -1.0, 1e-15));
  // ties: the first occurrence; the constant's minimum is the from point (its sensitivity that of the from point)
  o = win(CH_MEAS_MIN, 1, 0.5, 3.0);
  CHECK(o.st == MEAS_OK && o.v == -2.0 && o.d[0] == 1.0);
  // ends outside the run are clipped: [0, 4]: 24, average 6; ends on rows read the rows
  CHECK(near(win(CH_MEAS_INTEG, 0, -5.0, 100.0).v, 24.0, 1e-14) && near(win(CH_MEAS_AVG, 0, -INF, INF).v, 6.0, 1e-14));
  CHECK(near(win(CH_MEAS_INTEG, 0, 1.0, 2.0).v, 4.5, 1e-15) && win(CH_MEAS_MAX, 0, 1.0, 2.0).v == 6.0 && win(CH_MEAS_MIN, 0, 1.0, 2.0).d[0] == 1.0);
  // empty windows: from == to, from > to, wholly behind or in front of the run
  for (auto ft : {std::pair<double, double>{1.5, 1.5}, {2.0, 1.0}, {4.0, 9.0}, {5.0, 9.0}, {-3.0, 0.0}, {-3.0, -1.0}}) {
    o = win(CH_MEAS_AVG, 0, ft.first, ft.second);
    CHECK(o.st == MEAS_EMPTY && std::isnan(o.v) && std::isnan(o.d[0]));
  }
  // a repeated time inside the window: both rows are points, the jump has no area: t = 0 1 1 2, y = 0 1 3 3: 0.5 + 0 + 3; max 3 first at row 2
  Run j; j.t = {0, 1, 1, 2}; j.V = {0, 1, 3, 3}; j.n_par = 1; j.Sn = {0, 1, 2, 5};
  o = eval(j, spec(CH_MEAS_INTEG, side(0)));
  CHECK(o.st == MEAS_OK && near(o.v, 3.5, 1e-15) && near(o.d[0], 0.5 + 3.5, 1e-15));
  o = eval(j, spec(CH_MEAS_MAX, side(0)));
  CHECK(o.st == MEAS_OK && o.v == 3.0 && o.d[0] == 2.0);
  // a window that starts on the repeated time reads its later row, one that ends there the earlier
  CHECK(eval(j, spec(CH_MEAS_MIN, side(0), side(0), 0.0, 1.0, 2.0)).v == 3.0 && eval(j, spec(CH_MEAS_MAX, side(0), side(0), 0.0, 0.0, 1.0)).v == 1.0);
}

static void nan_rows() {
  Run r; r.t = {0, 1, 2, 3, 4}; r.V = {0, 1, QNAN, 3, 4};
  auto when = [&](int n) { return eval(r, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5, CH_EDGE_RISE, n))); };
  CHECK(when(1).st == MEAS_OK && near(when(1).v, 0.5, 1e-15));   // read rows 0 and 1 only
  CHECK(when(2).st == MEAS_NONFINITE && std::isnan(when(2).v));    // read to the end
  CHECK(when(CH_MEAS_LAST).st == MEAS_NONFINITE);                  // the last event is known only at the end
  auto win = [&](double from, double to) { return eval(r, spec(CH_MEAS_INTEG, side(0), side(0), 0.0, from, to)); };
  CHECK(win(0.0, 1.0).st == MEAS_OK && near(win(0.0, 1.0).v, 0.5, 1e-15));
  CHECK(win(0.0, 1.5).st == MEAS_NONFINITE && win(2.5, 4.0).st == MEAS_NONFINITE && win(0.0, 2.0).st == MEAS_NONFINITE);
  CHECK(win(3.0, 4.0).st == MEAS_OK && near(win(3.0, 4.0).v, 3.5, 1e-15));
  CHECK(eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), 3.5)).st == MEAS_OK && eval(r, spec(CH_MEAS_FIND_AT, side(0), side(0), 2.5)).st == MEAS_NONFINITE);
  r.V = {0, 1, INF, 3, 4};
  CHECK(when(2).st == MEAS_NONFINITE && win(0.0, 4.0).st == MEAS_NONFINITE && eval(r, spec(CH_MEAS_MAX, side(0))).st == MEAS_NONFINITE);
  Run one; one.t = {0.0}; one.V = {QNAN};
  CHECK(eval(one, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5))).st == MEAS_NONFINITE && eval(one, spec(CH_MEAS_FIND_AT, side(0))).st == MEAS_NONFINITE);
}

static void chunks_and_checks() {
  // samples per launch: all of them under the cap; whole wavefronts from 64 up; at least one
  CHECK(meas_sample_chunk(2, 100, 0, 1000, 1e9) == 1000);
  CHECK(meas_sample_chunk(2, 100, 0, 1000, 200.0 * 130) == 128);     // 130 fit: 2 wavefronts
  CHECK(meas_sample_chunk(2, 100, 1, 1000, 200.0 * 130) == 64);      // sensitivity rows of one parameter double a sample: 65 fit
  CHECK(meas_sample_chunk(2, 100, 0, 1000, 200.0 * 63) == 63 && meas_sample_chunk(2, 100, 0, 1000, 10.0) == 1);
  CHECK(meas_sample_chunk(0, 0, 0, 5, 8.0) == 5 && meas_sample_chunk(1, 1, 0, 5, 4.0) == 4);   // (no rows count as one double per sample)
  // the lanes' chunks tile the intervals 1 .. nt-1 in order
  for (long nt : {1L, 2L, 3L, 64L, 65L, 66L, 129L, 1000L}) {
    long next = 1; bool ok = true;
    for (int l = 0; l < 64; ++l) { long ia, ib; meas_lane_chunk(nt, l, ia, ib); ok = ok && ia == (next < nt ? next : nt) && ib >= ia && ib <= nt; next = ib > next ? ib : next; }
    CHECK(ok && next == (nt > 1 ? nt : 1));
  }
  { long ia, ib; meas_lane_chunk(129, 1, ia, ib); CHECK(ia == 3 && ib == 5); meas_lane_chunk(66, 32, ia, ib); CHECK(ia == 65 && ib == 66); meas_lane_chunk(66, 33, ia, ib); CHECK(ia == ib); }
  // refusals
  CHECK(meas_spec_check(spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5)), 1) == nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_WHEN, side(1, -1, 1.0, 0.5)), 1) != nullptr && meas_spec_check(spec(CH_MEAS_WHEN, side(0, 1, 1.0, 0.5)), 1) != nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5, CH_EDGE_RISE, 0)), 1) != nullptr && meas_spec_check(spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5, CH_EDGE_RISE, -2)), 1) != nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_WHEN, side(0, -1, 1.0, QNAN)), 1) != nullptr && meas_spec_check(spec(CH_MEAS_WHEN, side(0, -1, 1.0, INF)), 1) != nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_DELAY, side(0, -1, 1.0, 0.5), side(0, -1, 1.0, 0.5, CH_EDGE_RISE, 0)), 1) != nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_FIND_WHEN, side(0, -1, 1.0, 0.5), side(3)), 3) != nullptr && meas_spec_check(spec(CH_MEAS_FIND_WHEN, side(0, -1, 1.0, 0.5), side(2, -1, 1.0, QNAN, 0, 0)), 3) == nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_AVG, side(0, -1, 1.0, QNAN, 0, 0)), 1) == nullptr && meas_spec_check(spec(CH_MEAS_AVG, side(0), side(0), 0.0, QNAN, 1.0), 1) != nullptr);
  CHECK(meas_spec_check(spec(CH_MEAS_N_KINDS, side(0)), 1) != nullptr && meas_spec_check(spec(-1, side(0)), 1) != nullptr);
}

// ---- the wave form against the one-pass form on a longer run: 129 rows (2 intervals per lane), a wavy signal with dense points ----
static void wave_against_serial() {
  for (long nt : {1L, 2L, 3L, 64L, 65L, 66L, 129L}) {
    Run r; r.n_par = 2;
    for (long i = 0; i < nt; ++i) { r.t.push_back(0.1 * i + 0.03 * std::sin(1.7 * i)); r.pts.push_back((int32_t)(1 + i % 5)); }
    if (nt > 40) r.t[40] = r.t[39];   // a repeated time
    for (long i = 0; i < nt; ++i) r.V.push_back(std::sin(2.3 * r.t[i]) + 0.1 * r.t[i]);
    for (long i = 0; i < nt; ++i) r.V.push_back(std::cos(0.9 * r.t[i]));
    for (int q = 0; q < 4; ++q) for (long i = 0; i < nt; ++i) r.Sn.push_back(std::cos(1.1 * r.t[i] + q));
    if (nt == 129) r.V[4] = 0.5;   // row 4 closes lane 1's chunk [3, 5): an event ON the chunk boundary (y_i == L below)
    const double t_end = r.t[nt - 1];
    std::vector<ch_measure_spec> specs;
    for (int edge : {CH_EDGE_RISE, CH_EDGE_FALL, CH_EDGE_CROSS}) for (int n : {1, 2, 3, 7, CH_MEAS_LAST}) for (double td : {-INF, 0.37 * t_end}) {
      specs.push_back(spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5, edge, n, td)));
      specs.push_back(spec(CH_MEAS_DELAY, side(0, -1, 1.0, 0.5, edge, 1, td), side(1, 0, 2.0, 0.1, CH_EDGE_CROSS, n)));
      specs.push_back(spec(CH_MEAS_FIND_WHEN, side(0, 1, 1.0, 0.2, edge, n, td), side(1)));
    }
    // windows: the whole run, ends inside the first and the last chunk, a window inside one interval, an empty one
    for (int kind = CH_MEAS_FIND_AT; kind < CH_MEAS_N_KINDS; ++kind)
      for (auto ft : {std::pair<double, double>{-INF, INF}, {0.013 * t_end, 0.991 * t_end}, {0.5 * t_end, 0.5 * t_end + 0.01}, {0.4 * t_end, 0.4 * t_end}})
        specs.push_back(spec(kind, side(0, 1, 0.5), side(0), 0.3 * t_end, ft.first, ft.second));
    for (const ch_measure_spec& sp : specs) {
      const Out a = eval(r, sp), b = wave_eval(r, sp);
      CHECK(a.st == b.st);
      const bool sums = sp.kind == CH_MEAS_INTEG || sp.kind == CH_MEAS_AVG || sp.kind == CH_MEAS_RMS;
      if (!sums) CHECK(same_bits(a.v, b.v) && same_bits(a.d[0], b.d[0]) && same_bits(a.d[1], b.d[1]));
      else CHECK((a.st != MEAS_OK && std::isnan(b.v)) || (near(a.v, b.v, 1e-13 * (1.0 + t_end)) && near(a.d[0], b.d[0], 1e-13 * (1.0 + t_end)) && near(a.d[1], b.d[1], 1e-13 * (1.0 + t_end))));
    }
    if (nt == 129) {   // the boundary event is the first rise through 0.5 or comes behind earlier ones: it must be among the events found
      bool seen = false;
      for (int n = 1; n <= 4; ++n) { const Out o = wave_eval(r, spec(CH_MEAS_WHEN, side(0, -1, 1.0, 0.5, CH_EDGE_CROSS, n))); if (o.st == MEAS_OK && o.v == r.t[4]) seen = true; }
      CHECK(seen);
    }
  }
}

int main() {
  closed_forms();
  event_rules();
  windows();
  nan_rows();
  chunks_and_checks();
  wave_against_serial();
  std::printf("measure host: %d checks, %d bad\n", nchecked, nbad);
  return nbad == 0 ? 0 : 1;
}
