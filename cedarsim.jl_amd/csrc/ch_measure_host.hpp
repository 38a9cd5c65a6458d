// ch_measure_host.hpp — waveform measurements over a finished transient (.measure): the arithmetic of ONE (measure, sample) pair,
// host and device, nothing but <cmath>.  measure_lanes_kernel calls meas_eval as it stands; measure_wave_kernel
// (ch_measure_kernels.hpp) calls the same pieces on 64 chunks of the time axis and combines them; tests/host_measure.cpp runs them
// under ASan / UBSan.  DESIGN.md 2.7e has the definitions in words.
//
// Rows are [row][time][sample]: element (row, i) of one sample is base[(row * nt + i) * ld].  A signal is y_i = scale * (V[a][i] - V[b][i]).
// On (t_{i-1}, t_i] the signal is the polynomial solution._dense_eval evaluates: through the m = min(pts[i], i + 1) newest rows when
// m >= 2 and their times are distinct, else the line through rows i-1 and i (a line is the m = 2 polynomial: one code path); an
// interval of zero length (a restart repeats a time) has the value y_i.
#pragma once
#include <cmath>

#include "../../include/cedarhip.h"

#if defined(__HIPCC__)
#define CH_MEAS_HD __host__ __device__ inline
#else
#define CH_MEAS_HD inline
#endif
// First in the body of every function that does floating-point arithmetic here: no fused multiply-adds.  Each operation then rounds once,
// wherever the function is inlined: the two kernel forms, which call the same functions with the same arguments, give the same bits.
// (The device compiler and the library's host side are clang.  A host compiler without the pragma fuses nothing unless asked to.)
#if defined(__clang__)
#define CH_MEAS_NOCONTRACT _Pragma("STDC FP_CONTRACT OFF")
#else
#define CH_MEAS_NOCONTRACT
#endif

namespace chip {

constexpr int MEAS_MAX_PTS = 8;   // rows one dense-output polynomial runs through (order 5 uses 6); measure_check refuses more
enum { MEAS_OK = 0, MEAS_NOT_FOUND = 1, MEAS_EMPTY = 2, MEAS_NONFINITE = 3, MEAS_FLAT = 4 };

CH_MEAS_HD bool meas_finite(double x) { return (x - x) == 0.0; }
CH_MEAS_HD double meas_nan() { return CH_NAN; }

// the rows of one sample: times, dense points (or null), state rows and sensitivity rows (or null; row r, parameter k at r * n_par + k)
struct MeasRows {
  const double* t; const int32_t* pts; long nt;
  const double* V; long ldV;
  const double* Sn; long ldS; int n_par;
};
struct MeasSig {
  const double* a; const double* b; long ld; double scale;
  CH_MEAS_HD double at(long i) const { CH_MEAS_NOCONTRACT const double v = a[i * ld]; return scale * (b ? v - b[i * ld] : v); }
};
CH_MEAS_HD MeasSig meas_signal(const MeasRows& R, const ch_measure_side& sd, long s) {
  MeasSig y; y.ld = R.ldV; y.scale = sd.scale;
  y.a = R.V + (long)sd.row_a * R.nt * R.ldV + s; y.b = sd.row_b >= 0 ? R.V + (long)sd.row_b * R.nt * R.ldV + s : nullptr;
  return y;
}
CH_MEAS_HD MeasSig meas_sens_signal(const MeasRows& R, const ch_measure_side& sd, long s, int k) {
  MeasSig y; y.ld = R.ldS; y.scale = sd.scale;
  y.a = R.Sn + ((long)sd.row_a * R.n_par + k) * R.nt * R.ldS + s; y.b = sd.row_b >= 0 ? R.Sn + ((long)sd.row_b * R.n_par + k) * R.nt * R.ldS + s : nullptr;
  return y;
}

// ---- the interpolant ----
// rows i0 .. i0 + m - 1 of interval i >= 1; m = 1: zero length, the value is y_i
CH_MEAS_HD void meas_window(const double* t, const int32_t* pts, long i, long& i0, int& m) {
  if (!(t[i] > t[i - 1])) { i0 = i; m = 1; return; }
  long mm = pts ? (long)pts[i] : 0;
  if (mm > i + 1) mm = i + 1;
  if (mm > MEAS_MAX_PTS) mm = MEAS_MAX_PTS;
  // repeated times among the mm rows are counted, and both results are selected from the one flag (tests/test_gpu_measure.py reads
  // the window and its weights back from the device through unit rows)
  long repeated = 0;
  for (long a = i - mm + 2; a <= i; ++a) repeated += t[a] > t[a - 1] ? 0 : 1;
  const bool poly = mm >= 2 && repeated == 0;
  i0 = poly ? i - mm + 1 : i - 1;
  m = poly ? (int)mm : 2;
}
// Lagrange weights at x and their derivatives; at a node the weights are exactly 0 and 1
CH_MEAS_HD void meas_weights(const double* t, long i0, int m, double x, double* w) { CH_MEAS_NOCONTRACT
  for (int a = 0; a < m; ++a) {
    double p = 1.0;
    for (int b = 0; b < m; ++b) if (b != a) p *= (x - t[i0 + b]) / (t[i0 + a] - t[i0 + b]);
    w[a] = p;
  }
}
CH_MEAS_HD void meas_dweights(const double* t, long i0, int m, double x, double* dw) { CH_MEAS_NOCONTRACT
  for (int a = 0; a < m; ++a) {
    double sum = 0.0;
    for (int c = 0; c < m; ++c) if (c != a) {
      double p = 1.0 / (t[i0 + a] - t[i0 + c]);
      for (int b = 0; b < m; ++b) if (b != a && b != c) p *= (x - t[i0 + b]) / (t[i0 + a] - t[i0 + b]);
      sum += p;
    }
    dw[a] = sum;
  }
}
CH_MEAS_HD double meas_dot(const MeasSig& y, long i0, int m, const double* w) { CH_MEAS_NOCONTRACT
  double acc = 0.0;
  for (int a = 0; a < m; ++a) acc += w[a] * y.at(i0 + a);
  return acc;
}
CH_MEAS_HD bool meas_rows_finite(const MeasSig& y, long i0, int m) {
  bool ok = true;
  for (int a = 0; a < m; ++a) ok = ok && meas_finite(y.at(i0 + a));
  return ok;
}
// where a time sits: x <= t_0 is row 0, x >= t_last the last row, else the interval (t_{i-1}, t_i] with the first t_i >= x
struct MeasAt { long i0; int m; double w[MEAS_MAX_PTS]; };
CH_MEAS_HD void meas_locate(const double* t, const int32_t* pts, long nt, double x, MeasAt& p) { CH_MEAS_NOCONTRACT
  p.m = 1; p.w[0] = 1.0;
  if (!(x > t[0])) { p.i0 = 0; return; }
  if (!(x < t[nt - 1])) { p.i0 = nt - 1; return; }
  long lo = 0, hi = nt - 1;   // t[lo] < x <= t[hi]
  while (hi - lo > 1) { const long mid = lo + (hi - lo) / 2; if (t[mid] >= x) hi = mid; else lo = mid; }
  meas_window(t, pts, hi, p.i0, p.m);
  meas_weights(t, p.i0, p.m, x, p.w);
}

// ---- events ----
// rise: y_{i-1} < L <= y_i; fall: y_{i-1} > L >= y_i (a touch from one side is no event; NaN rows are none)
CH_MEAS_HD bool meas_is_event(double y0, double y1, double L, int edge) {
  const bool rise = y0 < L && L <= y1, fall = y0 > L && L >= y1;
  return ((edge & CH_EDGE_RISE) && rise) || ((edge & CH_EDGE_FALL) && fall);
}
// The event's time in interval i: t_i when y_i == L or the interval has no length, else a root of P - L by bisection on the
// bracket [t_{i-1}, t_i] (signs taken from the rows) until the bracket no longer shrinks; the upper end is returned.
CH_MEAS_HD double meas_event_time(const double* t, const int32_t* pts, const MeasSig& y, long i, double L) { CH_MEAS_NOCONTRACT
  const double y0 = y.at(i - 1), y1 = y.at(i);
  if (y1 == L || !(t[i] > t[i - 1])) return t[i];
  long i0; int m; double w[MEAS_MAX_PTS];
  meas_window(t, pts, i, i0, m);
  const bool up = y0 < L;
  double lo = t[i - 1], hi = t[i];
  for (int it = 0; it < 256; ++it) {
    const double mid = lo + 0.5 * (hi - lo);
    if (!(mid > lo) || !(mid < hi)) break;
    meas_weights(t, i0, m, mid, w);
    const double g = meas_dot(y, i0, m, w) - L;
    if (g == 0.0) return mid;
    if ((g < 0.0) == up) lo = mid; else hi = mid;
  }
  return hi;
}
// One pass over intervals [ia, ib): events at or after td counted; `want` > 0 stops at the want-th and reports it in hit.
// first_nf: the first non-finite row among those read (nt: none).  An interval that ends before td cannot hold a counted event; one
// that starts at or after td (or has no length and sits at or after td) always does; only the interval td falls into is solved here.
struct MeasScan { long count, hit, last, first_nf; };
CH_MEAS_HD MeasScan meas_scan(const MeasRows& R, const MeasSig& y, const ch_measure_side& sd, long ia, long ib, long want) {
  MeasScan r; r.count = 0; r.hit = -1; r.last = -1; r.first_nf = R.nt;
  if (ia >= ib) return r;
  const double* t = R.t;
  double y0 = y.at(ia - 1);
  if (ia == 1 && !meas_finite(y0)) r.first_nf = 0;
  for (long i = ia; i < ib; ++i) {
    const double y1 = y.at(i);
    if (!meas_finite(y1) && r.first_nf == R.nt) r.first_nf = i;
    if (t[i] >= sd.td && meas_is_event(y0, y1, sd.level, sd.edge)) {
      bool counts = t[i - 1] >= sd.td || !(t[i] > t[i - 1]);
      if (!counts) counts = meas_event_time(t, R.pts, y, i, sd.level) >= sd.td;
      if (counts) { ++r.count; r.last = i; if (r.count == want) { r.hit = i; return r; } }
    }
    y0 = y1;
  }
  return r;
}
// the event in interval i: its time, the interpolation weights there and P'(t*) of the event's own signal
struct MeasEvent { long i, i0; int m; double t, dP; double w[MEAS_MAX_PTS]; };
CH_MEAS_HD void meas_event_at(const MeasRows& R, const MeasSig& y, long i, double L, MeasEvent& e) { CH_MEAS_NOCONTRACT
  e.i = i; e.t = meas_event_time(R.t, R.pts, y, i, L);
  meas_window(R.t, R.pts, i, e.i0, e.m);
  meas_weights(R.t, e.i0, e.m, e.t, e.w);
  double dw[MEAS_MAX_PTS];
  meas_dweights(R.t, e.i0, e.m, e.t, dw);
  e.dP = e.m > 1 ? meas_dot(y, e.i0, e.m, dw) : 0.0;
}
CH_MEAS_HD bool meas_event_flat(const MeasEvent& e) { return e.m > 1 && !(e.dP != 0.0 && meas_finite(e.dP)); }
// d t*/d p = -P_s(t*) / P'(t*); 0 where the jump sits at a fixed break point
CH_MEAS_HD double meas_event_dtdp(const MeasEvent& e, const MeasSig& s) { CH_MEAS_NOCONTRACT return e.m == 1 ? 0.0 : -meas_dot(s, e.i0, e.m, e.w) / e.dP; }

// What an event search found: the interval (or -1) and whether a non-finite row sits in the span it read: rows 0 .. i for the n-th
// event, every row for the last one and when nothing was found.  meas_search is the whole time axis in one pass; the wave form
// builds the same record from 64 scans.
struct MeasFound { long i; bool nonfinite; };
CH_MEAS_HD MeasFound meas_found(const ch_measure_side& sd, long i, long first_nf, long nt) {
  MeasFound f; f.i = i;
  f.nonfinite = (sd.count > 0 && i >= 0) ? first_nf <= i : first_nf < nt;
  return f;
}
CH_MEAS_HD MeasFound meas_search(const MeasRows& R, const MeasSig& y, const ch_measure_side& sd) {
  const MeasScan sc = meas_scan(R, y, sd, 1, R.nt, sd.count > 0 ? (long)sd.count : 0);
  const long first_nf = (R.nt == 1 && !meas_finite(y.at(0))) ? 0 : sc.first_nf;
  return meas_found(sd, sd.count > 0 ? sc.hit : sc.last, first_nf, R.nt);
}
// WHEN, DELAY, FIND_WHEN from the searches' records: value, status and d/dp_k into sens[k * stride] (sens may be null)
CH_MEAS_HD int meas_finish_event(const MeasRows& R, const ch_measure_spec& sp, long s, MeasFound f1, MeasFound f2, double* value, double* sens, long stride) { CH_MEAS_NOCONTRACT
  const int np = (sens && R.Sn) ? R.n_par : 0;
  const bool two = sp.kind == CH_MEAS_DELAY;
  int st = MEAS_OK;
  if (f1.nonfinite || (two && f2.nonfinite)) st = MEAS_NONFINITE;
  else if (f1.i < 0 || (two && f2.i < 0)) st = MEAS_NOT_FOUND;
  MeasEvent e1, e2;
  const MeasSig y1 = meas_signal(R, sp.s1, s), y2 = meas_signal(R, sp.s2, s);
  if (st == MEAS_OK) {
    meas_event_at(R, y1, f1.i, sp.s1.level, e1);
    if (two) meas_event_at(R, y2, f2.i, sp.s2.level, e2);
    if (sp.kind == CH_MEAS_FIND_WHEN && !meas_rows_finite(y2, e1.i0, e1.m)) st = MEAS_NONFINITE;
  }
  if (st != MEAS_OK) {
    *value = meas_nan();
    for (int k = 0; k < np; ++k) sens[k * stride] = meas_nan();
    return st;
  }
  if (meas_event_flat(e1) || (two && meas_event_flat(e2))) st = MEAS_FLAT;
  double dP2 = 0.0;
  if (sp.kind == CH_MEAS_WHEN) *value = e1.t;
  else if (two) *value = e2.t - e1.t;
  else {
    *value = meas_dot(y2, e1.i0, e1.m, e1.w);
    double dw[MEAS_MAX_PTS];
    meas_dweights(R.t, e1.i0, e1.m, e1.t, dw);
    dP2 = e1.m > 1 ? meas_dot(y2, e1.i0, e1.m, dw) : 0.0;
  }
  for (int k = 0; k < np; ++k) {
    double d = meas_nan();
    if (st == MEAS_OK) {
      const double d1 = meas_event_dtdp(e1, meas_sens_signal(R, sp.s1, s, k));
      if (sp.kind == CH_MEAS_WHEN) d = d1;
      else if (two) d = meas_event_dtdp(e2, meas_sens_signal(R, sp.s2, s, k)) - d1;
      else d = meas_dot(meas_sens_signal(R, sp.s2, s, k), e1.i0, e1.m, e1.w) + dP2 * d1;
    }
    sens[k * stride] = d;
  }
  return st;
}
CH_MEAS_HD int meas_find_at(const MeasRows& R, const ch_measure_spec& sp, long s, double* value, double* sens, long stride) { CH_MEAS_NOCONTRACT
  const int np = (sens && R.Sn) ? R.n_par : 0;
  const MeasSig y = meas_signal(R, sp.s1, s);
  MeasAt p;
  meas_locate(R.t, R.pts, R.nt, sp.at, p);
  const bool ok = meas_rows_finite(y, p.i0, p.m);
  *value = ok ? meas_dot(y, p.i0, p.m, p.w) : meas_nan();
  for (int k = 0; k < np; ++k) sens[k * stride] = ok ? meas_dot(meas_sens_signal(R, sp.s1, s, k), p.i0, p.m, p.w) : meas_nan();
  return ok ? MEAS_OK : MEAS_NONFINITE;
}

// ---- windows ----
// [from, to] clipped to the run.  The point set (from, the rows strictly inside, to) is walked interval by interval: interval i gives
// the piece [max(t_{i-1}, from), min(t_i, to)] with row values at row times and the interpolant at from / to.  Keys order the points
// in time for "first occurrence": -1 the from point, i row i, nt the to point.
struct MeasAcc {
  double integ, sq, integ_s, ys, mn, mx; long kmn, kmx; bool nonfinite;
  CH_MEAS_HD void clear() { integ = sq = integ_s = ys = 0.0; mn = HUGE_VAL; mx = -HUGE_VAL; kmn = kmx = 0x7fffffffffffffffL; nonfinite = false; }
  CH_MEAS_HD void point(double v, long key) {
    if (v < mn || (v == mn && key < kmn)) { mn = v; kmn = key; }
    if (v > mx || (v == mx && key < kmx)) { mx = v; kmx = key; }
  }
  // `o` holds later points than this
  CH_MEAS_HD void add(const MeasAcc& o) {
    integ += o.integ; sq += o.sq; integ_s += o.integ_s; ys += o.ys; nonfinite = nonfinite || o.nonfinite;
    if (o.mn < mn || (o.mn == mn && o.kmn < kmn)) { mn = o.mn; kmn = o.kmn; }
    if (o.mx > mx || (o.mx == mx && o.kmx < kmx)) { mx = o.mx; kmx = o.kmx; }
  }
};
CH_MEAS_HD void meas_clip(const MeasRows& R, const ch_measure_spec& sp, double& from, double& to) {
  from = sp.from > R.t[0] ? sp.from : R.t[0];
  to = sp.to < R.t[R.nt - 1] ? sp.to : R.t[R.nt - 1];
}
// intervals [ia, ib) into acc; sn: the sensitivity rows of one parameter (integ_s, ys), or null
CH_MEAS_HD void meas_window_chunk(const MeasRows& R, const MeasSig& y, const MeasSig* sn, double from, double to, long ia, long ib, MeasAcc& acc) { CH_MEAS_NOCONTRACT
  const double* t = R.t;
  double w[MEAS_MAX_PTS];
  for (long i = ia; i < ib; ++i) {
    const double ta = t[i - 1], tb = t[i];
    if (!(tb > from)) continue;
    if (!(ta < to)) break;
    double xa = ta, xb = tb, ya = y.at(i - 1), yb = y.at(i), sa = sn ? sn->at(i - 1) : 0.0, sb = sn ? sn->at(i) : 0.0;
    if (from > ta || to < tb) {
      long i0; int m;
      meas_window(t, R.pts, i, i0, m);
      if (!meas_rows_finite(y, i0, m)) acc.nonfinite = true;
      if (from > ta) { xa = from; meas_weights(t, i0, m, from, w); ya = meas_dot(y, i0, m, w); if (sn) sa = meas_dot(*sn, i0, m, w); }
      if (to < tb) { xb = to; meas_weights(t, i0, m, to, w); yb = meas_dot(y, i0, m, w); if (sn) sb = meas_dot(*sn, i0, m, w); }
    }
    if (!meas_finite(ya) || !meas_finite(yb)) acc.nonfinite = true;
    const double h = xb - xa;
    acc.integ += 0.5 * (ya + yb) * h; acc.sq += 0.5 * (ya * ya + yb * yb) * h;
    acc.integ_s += 0.5 * (sa + sb) * h; acc.ys += 0.5 * (ya * sa + yb * sb) * h;
    if (from >= ta) acc.point(ya, -1);
    acc.point(yb, to < tb ? R.nt : i);
  }
}
CH_MEAS_HD int meas_window_value(int kind, const MeasAcc& a, double from, double to, double* value) { CH_MEAS_NOCONTRACT
  if (!(to > from)) { *value = meas_nan(); return MEAS_EMPTY; }
  if (a.nonfinite) { *value = meas_nan(); return MEAS_NONFINITE; }
  switch (kind) {
    case CH_MEAS_INTEG: *value = a.integ; break;
    case CH_MEAS_AVG: *value = a.integ / (to - from); break;
    case CH_MEAS_RMS: *value = std::sqrt(a.sq / (to - from)); break;
    case CH_MEAS_MIN: *value = a.mn; break;
    case CH_MEAS_MAX: *value = a.mx; break;
    default: *value = a.mx - a.mn; break;
  }
  return MEAS_OK;
}
// Where an end of a non-empty clipped window sits, as meas_window_chunk reads it: `from` in the interval with t_{i-1} <= from < t_i,
// `to` in the one with t_{i-1} < to <= t_i; an end on a row's time is that row (the later row of a repeated time at from, the
// earlier at to: the window lies between them).
CH_MEAS_HD void meas_locate_end(const double* t, const int32_t* pts, long nt, double x, bool is_from, MeasAt& p) { CH_MEAS_NOCONTRACT
  long lo = 0, hi = nt - 1;   // from: t[lo] <= x < t[hi]; to: t[lo] < x <= t[hi]
  while (hi - lo > 1) { const long mid = lo + (hi - lo) / 2; if (is_from ? t[mid] > x : t[mid] >= x) hi = mid; else lo = mid; }
  p.m = 1; p.w[0] = 1.0;
  if (is_from && t[hi - 1] == x) { p.i0 = hi - 1; return; }
  if (!is_from && t[hi] == x) { p.i0 = hi; return; }
  meas_window(t, pts, hi, p.i0, p.m);
  meas_weights(t, p.i0, p.m, x, p.w);
}
// the sensitivity rows of one parameter at the point with this key
CH_MEAS_HD double meas_sens_at_key(const MeasRows& R, const MeasSig& sn, long key, double from, double to) {
  if (key >= 0 && key < R.nt) return sn.at(key);
  MeasAt p;
  meas_locate_end(R.t, R.pts, R.nt, key < 0 ? from : to, key < 0, p);
  return meas_dot(sn, p.i0, p.m, p.w);
}
// a: the accumulation with parameter k's rows as sn
CH_MEAS_HD double meas_window_sens(int kind, const MeasRows& R, const MeasSig& sn, const MeasAcc& a, double from, double to) { CH_MEAS_NOCONTRACT
  switch (kind) {
    case CH_MEAS_INTEG: return a.integ_s;
    case CH_MEAS_AVG: return a.integ_s / (to - from);
    case CH_MEAS_RMS: return a.ys / (std::sqrt(a.sq / (to - from)) * (to - from));
    case CH_MEAS_MIN: return meas_sens_at_key(R, sn, a.kmn, from, to);
    case CH_MEAS_MAX: return meas_sens_at_key(R, sn, a.kmx, from, to);
    default: return meas_sens_at_key(R, sn, a.kmx, from, to) - meas_sens_at_key(R, sn, a.kmn, from, to);
  }
}

// ---- one (measure, sample), the whole time axis in one pass: returns the status ----
CH_MEAS_HD int meas_eval(const MeasRows& R, const ch_measure_spec& sp, long s, double* value, double* sens, long stride) {
  if (sp.kind == CH_MEAS_WHEN || sp.kind == CH_MEAS_DELAY || sp.kind == CH_MEAS_FIND_WHEN) {
    const MeasFound f1 = meas_search(R, meas_signal(R, sp.s1, s), sp.s1);
    MeasFound f2; f2.i = -1; f2.nonfinite = false;
    if (sp.kind == CH_MEAS_DELAY) f2 = meas_search(R, meas_signal(R, sp.s2, s), sp.s2);
    return meas_finish_event(R, sp, s, f1, f2, value, sens, stride);
  }
  if (sp.kind == CH_MEAS_FIND_AT) return meas_find_at(R, sp, s, value, sens, stride);
  const int np = (sens && R.Sn) ? R.n_par : 0;
  const MeasSig y = meas_signal(R, sp.s1, s);
  double from, to;
  meas_clip(R, sp, from, to);
  MeasAcc a; a.clear();
  meas_window_chunk(R, y, nullptr, from, to, 1, R.nt, a);
  const int st = meas_window_value(sp.kind, a, from, to, value);
  for (int k = 0; k < np; ++k) {
    if (st != MEAS_OK) { sens[k * stride] = meas_nan(); continue; }
    const MeasSig sn = meas_sens_signal(R, sp.s1, s, k);
    MeasAcc ak; ak.clear();
    meas_window_chunk(R, y, &sn, from, to, 1, R.nt, ak);
    sens[k * stride] = meas_window_sens(sp.kind, R, sn, ak, from, to);
  }
  return st;
}

// ---- what the engine checks before anything is uploaded: null, or why the spec is refused ----
CH_MEAS_HD bool meas_uses_s2(int kind) { return kind == CH_MEAS_DELAY || kind == CH_MEAS_FIND_WHEN; }
CH_MEAS_HD bool meas_is_event_kind(int kind) { return kind == CH_MEAS_WHEN || kind == CH_MEAS_DELAY || kind == CH_MEAS_FIND_WHEN; }
CH_MEAS_HD const char* meas_side_check(const ch_measure_side& sd, int n_rows, bool event) {
  if (sd.row_a < 0 || sd.row_a >= n_rows || sd.row_b < -1 || sd.row_b >= n_rows) return "a row out of range";
  if (!meas_finite(sd.scale)) return "a non-finite scale";
  if (!event) return nullptr;
  if (!meas_finite(sd.level)) return "a non-finite level";
  if (sd.count == 0 || sd.count < CH_MEAS_LAST) return "an event count of 0 (n >= 1, or CH_MEAS_LAST)";
  if (sd.edge < CH_EDGE_RISE || sd.edge > CH_EDGE_CROSS) return "an unknown edge";
  if (sd.td != sd.td) return "a NaN td";
  return nullptr;
}
CH_MEAS_HD const char* meas_spec_check(const ch_measure_spec& sp, int n_rows) {
  if (sp.kind < 0 || sp.kind >= CH_MEAS_N_KINDS) return "an unknown kind";
  const char* why = meas_side_check(sp.s1, n_rows, meas_is_event_kind(sp.kind));
  if (!why && meas_uses_s2(sp.kind)) why = meas_side_check(sp.s2, n_rows, sp.kind == CH_MEAS_DELAY);
  if (why) return why;
  if (sp.kind == CH_MEAS_FIND_AT && sp.at != sp.at) return "a NaN time";
  if (sp.kind >= CH_MEAS_INTEG && (sp.from != sp.from || sp.to != sp.to)) return "a NaN window";
  return nullptr;
}

// ---- sample chunks: when the rows the specs use (states and sensitivities) exceed `cap` doubles, the samples go in chunks of this
// many (at least 1; whole wavefronts from 64 up).  A sample's arithmetic never reads another sample, so its result does not depend on its chunk.
CH_MEAS_HD long meas_sample_chunk(long n_used_rows, long n_times, long n_par, long n_samples, double cap) {
  const double per = (double)(n_used_rows > 0 ? n_used_rows : 1) * (double)(n_times > 0 ? n_times : 1) * (double)(1 + (n_par > 0 ? n_par : 0));
  if (per * (double)n_samples <= cap) return n_samples > 0 ? n_samples : 1;
  long c = (long)(cap / per);
  if (c >= 64) c -= c % 64;
  return c < 1 ? 1 : c;
}
// intervals 1 .. nt-1 in 64 contiguous chunks: lane l of the wave form takes [ia, ib)
CH_MEAS_HD void meas_lane_chunk(long nt, int lane, long& ia, long& ib) {
  const long ni = nt - 1, per = (ni + 63) / 64;
  ia = 1 + (long)lane * per; ib = ia + per;
  if (ia > nt) ia = nt;
  if (ib > nt) ib = nt;
}

}  // namespace chip
