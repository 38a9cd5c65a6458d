// ch_fmeasure_host.hpp — frequency-domain measurements over an AC or noise result (.measure ac / noise): the arithmetic of ONE
// (measure, sample) pair, host and device, nothing but <cmath>.  fmeasure_lanes_kernel calls fmeas_eval as it stands;
// fmeasure_wave_kernel (ch_fmeasure_kernels.hpp) calls the same pieces on 64 chunks of the frequency axis and combines them;
// tests/host_fmeasure.cpp runs them under ASan / UBSan.  DESIGN.md 2.7g has the definitions in words.
//
// Rows are complex, [row][freq][sample][2]: element (row, i) of one sample is base[((row * nf + i) * ld) * 2 + {0, 1}].  A side reads
// H_i = scale * (X[a][i] - X[b][i]) and the real signal g_i = sig(H_i); PHASE is unwrapped along the grid from row 0 with an INTEGER
// wrap count k_i (the split form prefix-sums it exactly).  Between rows g is the line in (u, g), u = log10 f or f.
#pragma once
#include <cmath>

#include "ch_measure_host.hpp"

namespace chip {

enum { FMEAS_NO_OP = 5 };

CH_MEAS_HD bool fmeas_is_event_kind(int kind) { return kind == CH_FMEAS_WHEN || kind == CH_FMEAS_FIND_WHEN; }
CH_MEAS_HD bool fmeas_uses_s2(int kind) { return kind == CH_FMEAS_FIND_WHEN; }
// the transient kind with the same window arithmetic (meas_window_value / MeasAcc of ch_measure_host.hpp)
CH_MEAS_HD int fmeas_window_kind(int kind) { return kind - CH_FMEAS_INTEG + CH_MEAS_INTEG; }

// the rows of one launch: frequencies, their log10 (null when no spec asks for it), values and sensitivity rows (or null; row r,
// parameter k at r * n_par + k); ld in complex elements
struct FRows {
  const double* f; const double* ulog; long nf;
  const double* H; long ldH;
  const double* dH; long ldS; int n_par;
  CH_MEAS_HD const double* u(int xscale) const { return xscale == CH_FX_LOG ? ulog : f; }
};
CH_MEAS_HD double fmeas_u_of(int xscale, double f) { return xscale == CH_FX_LOG ? std::log10(f) : f; }
CH_MEAS_HD double fmeas_f_of(int xscale, double u) { return xscale == CH_FX_LOG ? std::pow(10.0, u) : u; }

struct FSig {
  const double* a; const double* b; long ld; double scale; int sig;
  CH_MEAS_HD void h(long i, double& re, double& im) const { CH_MEAS_NOCONTRACT
    re = a[2 * i * ld]; im = a[2 * i * ld + 1];
    if (b) { re = re - b[2 * i * ld]; im = im - b[2 * i * ld + 1]; }
    re = scale * re; im = scale * im;
  }
  // the signal without its wraps
  CH_MEAS_HD double raw(long i) const { CH_MEAS_NOCONTRACT
    double re, im;
    h(i, re, im);
    switch (sig) {
      case CH_FSIG_RE: return re;
      case CH_FSIG_IM: return im;
      case CH_FSIG_MAG: return std::sqrt(re * re + im * im);
      case CH_FSIG_DB: return 20.0 * std::log10(std::sqrt(re * re + im * im));
      case CH_FSIG_DB10: return 10.0 * std::log10(re);
      default: return (re == 0.0 && im == 0.0) ? meas_nan() : std::atan2(im, re) * (180.0 / 3.14159265358979323846);
    }
  }
  // the step of k from a row to the next: the raw increment leaves (-180, 180]
  CH_MEAS_HD long wrap(double r0, double r1) const { CH_MEAS_NOCONTRACT
    if (sig != CH_FSIG_PHASE) return 0;
    const double d = r1 - r0;
    return d > 180.0 ? -1 : (d <= -180.0 ? 1 : 0);
  }
  CH_MEAS_HD double val(double r, long k) const { CH_MEAS_NOCONTRACT return sig == CH_FSIG_PHASE ? r + 360.0 * (double)k : r; }
  // the wraps of rows ia .. ib-1 (each against the row before it): k_{ib-1} - k_{ia-1}
  CH_MEAS_HD long kcount(long ia, long ib) const {
    if (sig != CH_FSIG_PHASE || ia >= ib) return 0;
    long k = 0;
    double r0 = raw(ia - 1);
    for (long i = ia; i < ib; ++i) { const double r1 = raw(i); k += wrap(r0, r1); r0 = r1; }
    return k;
  }
  // d g_i / d p from the sensitivity rows `sn` of one parameter (same rows, same scale)
  CH_MEAS_HD double d(const FSig& sn, long i) const { CH_MEAS_NOCONTRACT
    double re, im, dre, dim;
    h(i, re, im); sn.h(i, dre, dim);
    const double m2 = re * re + im * im;
    switch (sig) {
      case CH_FSIG_RE: return dre;
      case CH_FSIG_IM: return dim;
      case CH_FSIG_MAG: return (re * dre + im * dim) / std::sqrt(m2);
      case CH_FSIG_DB: return (20.0 / 2.302585092994045684) * (re * dre + im * dim) / m2;
      case CH_FSIG_DB10: return (10.0 / 2.302585092994045684) * dre / re;
      default: return (180.0 / 3.14159265358979323846) * (re * dim - im * dre) / m2;
    }
  }
};
CH_MEAS_HD FSig fmeas_signal(const FRows& R, const ch_fmeasure_side& sd, long s) {
  FSig y; y.ld = R.ldH; y.scale = sd.scale; y.sig = sd.sig;
  y.a = R.H + ((long)sd.row_a * R.nf * R.ldH + s) * 2; y.b = sd.row_b >= 0 ? R.H + ((long)sd.row_b * R.nf * R.ldH + s) * 2 : nullptr;
  return y;
}
CH_MEAS_HD FSig fmeas_sens_signal(const FRows& R, const ch_fmeasure_side& sd, long s, int k) {
  FSig y; y.ld = R.ldS; y.scale = sd.scale; y.sig = sd.sig;
  y.a = R.dH + (((long)sd.row_a * R.n_par + k) * R.nf * R.ldS + s) * 2;
  y.b = sd.row_b >= 0 ? R.dH + (((long)sd.row_b * R.n_par + k) * R.nf * R.ldS + s) * 2 : nullptr;
  return y;
}

// ---- the interpolant ----
// a place on the axis: row i0 alone (m = 1), or rows i0, i0 + 1 with weights w0, w1 (exactly 0 and 1 at a row)
struct FAt { long i0; int m; double w0, w1; CH_MEAS_HD long upper() const { return i0 + m - 1; } };
CH_MEAS_HD void fmeas_weights(const double* u, long i, double x, FAt& p) { CH_MEAS_NOCONTRACT   // interval (u_{i-1}, u_i]
  p.i0 = i - 1; p.m = 2;
  p.w0 = (u[i] - x) / (u[i] - u[i - 1]); p.w1 = (x - u[i - 1]) / (u[i] - u[i - 1]);
}
// x <= u_0 is row 0, x >= u_last the last row, else the interval (u_{i-1}, u_i] with the first u_i >= x
CH_MEAS_HD void fmeas_locate(const double* u, long nf, double x, FAt& p) {
  p.m = 1; p.w0 = 1.0; p.w1 = 0.0;
  if (!(x > u[0])) { p.i0 = 0; return; }
  if (!(x < u[nf - 1])) { p.i0 = nf - 1; return; }
  long lo = 0, hi = nf - 1;   // u[lo] < x <= u[hi]
  while (hi - lo > 1) { const long mid = lo + (hi - lo) / 2; if (u[mid] >= x) hi = mid; else lo = mid; }
  fmeas_weights(u, hi, x, p);
}
// g there; kup: the wrap count of the upper row.  ok: every row read is finite
CH_MEAS_HD double fmeas_val_at(const FSig& y, const FAt& p, long kup, bool& ok) { CH_MEAS_NOCONTRACT
  if (p.m == 1) { const double g = y.val(y.raw(p.i0), kup); ok = meas_finite(g); return g; }
  const double r0 = y.raw(p.i0), r1 = y.raw(p.i0 + 1);
  const double g0 = y.val(r0, kup - y.wrap(r0, r1)), g1 = y.val(r1, kup);
  ok = meas_finite(g0) && meas_finite(g1);
  return p.w0 * g0 + p.w1 * g1;
}
CH_MEAS_HD double fmeas_slope_at(const FSig& y, const double* u, const FAt& p, long kup) { CH_MEAS_NOCONTRACT
  if (p.m == 1) return 0.0;
  const double r0 = y.raw(p.i0), r1 = y.raw(p.i0 + 1);
  return (y.val(r1, kup) - y.val(r0, kup - y.wrap(r0, r1))) / (u[p.i0 + 1] - u[p.i0]);
}
CH_MEAS_HD double fmeas_d_at(const FSig& y, const FSig& sn, const FAt& p) { CH_MEAS_NOCONTRACT
  return p.m == 1 ? y.d(sn, p.i0) : p.w0 * y.d(sn, p.i0) + p.w1 * y.d(sn, p.i0 + 1);
}

// ---- the level: absolute, or relative to the signal's own value at ref_at ----
struct FLevel { bool rel, bad; FAt p; double L; };
CH_MEAS_HD bool fmeas_level_rel(const ch_fmeasure_side& sd) { return meas_finite(sd.ref_at); }
CH_MEAS_HD void fmeas_level_locate(const FRows& R, int xscale, const ch_fmeasure_side& sd, FLevel& lv) {
  lv.rel = fmeas_level_rel(sd); lv.bad = false; lv.L = sd.level;
  lv.p.i0 = 0; lv.p.m = 1; lv.p.w0 = 1.0; lv.p.w1 = 0.0;
  if (lv.rel) fmeas_locate(R.u(xscale), R.nf, fmeas_u_of(xscale, sd.ref_at), lv.p);
}
// kref: the wrap count of lv.p.upper()
CH_MEAS_HD void fmeas_level_value(const FSig& y, const ch_fmeasure_side& sd, long kref, FLevel& lv) { CH_MEAS_NOCONTRACT
  if (!lv.rel) return;
  bool ok;
  const double g = fmeas_val_at(y, lv.p, kref, ok);
  lv.bad = !ok; lv.L = sd.level + g;
}

// ---- events ----
// rise: g_{i-1} < L <= g_i; fall: g_{i-1} > L >= g_i (a touch from one side is no event; NaN rows are none)
CH_MEAS_HD bool fmeas_is_event(double g0, double g1, double L, int edge) {
  const bool rise = g0 < L && L <= g1, fall = g0 > L && L >= g1;
  return ((edge & CH_EDGE_RISE) && rise) || ((edge & CH_EDGE_FALL) && fall);
}
// the event's abscissa in interval i: u_i when g_i == L, else where the line crosses L, kept inside the interval
CH_MEAS_HD double fmeas_event_u(const double* u, long i, double g0, double g1, double L) { CH_MEAS_NOCONTRACT
  if (g1 == L) return u[i];
  double x = u[i - 1] + (L - g0) / (g1 - g0) * (u[i] - u[i - 1]);
  if (!(x > u[i - 1])) x = u[i - 1];
  if (!(x < u[i])) x = u[i];
  return x;
}
CH_MEAS_HD double fmeas_event_f(const FRows& R, int xscale, long i, double g0, double g1, double L) {
  const double* u = R.u(xscale);
  const double x = fmeas_event_u(u, i, g0, g1, L);
  return x == u[i] ? R.f[i] : (x == u[i - 1] ? R.f[i - 1] : fmeas_f_of(xscale, x));
}
// One pass over intervals [ia, ib), k0 the wrap count of row ia - 1: events at or after fd counted; `want` > 0 stops at the want-th.
// khit / klast: the wrap count of the event's upper row.  first_nf: the first non-finite row among those read (nf: none).
struct FScan { long count, hit, last, first_nf, khit, klast; };
CH_MEAS_HD FScan fmeas_scan(const FRows& R, int xscale, const FSig& y, const ch_fmeasure_side& sd, double L, long ia, long ib, long k0, long want) {
  FScan r; r.count = 0; r.hit = -1; r.last = -1; r.first_nf = R.nf; r.khit = 0; r.klast = 0;
  if (ia >= ib) return r;
  double r0 = y.raw(ia - 1);
  long k = k0;
  double g0 = y.val(r0, k);
  if (ia == 1 && !meas_finite(g0)) r.first_nf = 0;
  for (long i = ia; i < ib; ++i) {
    const double r1 = y.raw(i);
    k += y.wrap(r0, r1);
    const double g1 = y.val(r1, k);
    if (!meas_finite(g1) && r.first_nf == R.nf) r.first_nf = i;
    if (R.f[i] >= sd.fd && fmeas_is_event(g0, g1, L, sd.edge)) {
      const bool counts = R.f[i - 1] >= sd.fd || fmeas_event_f(R, xscale, i, g0, g1, L) >= sd.fd;
      if (counts) { ++r.count; r.last = i; r.klast = k; if (r.count == want) { r.hit = i; r.khit = k; return r; } }
    }
    r0 = r1; g0 = g1;
  }
  return r;
}
// What an event search found: the interval (or -1), the wrap count of its upper row and whether a non-finite row sits in the span it
// read: rows 0 .. i for the n-th event, every row for the last one and when nothing was found.
struct FFound { long i, k; bool nonfinite; };
CH_MEAS_HD FFound fmeas_found(const ch_fmeasure_side& sd, long i, long k, long first_nf, long nf) {
  FFound f; f.i = i; f.k = k;
  f.nonfinite = (sd.count > 0 && i >= 0) ? first_nf <= i : first_nf < nf;
  return f;
}
CH_MEAS_HD FFound fmeas_search(const FRows& R, int xscale, const FSig& y, const ch_fmeasure_side& sd, double L) {
  const FScan sc = fmeas_scan(R, xscale, y, sd, L, 1, R.nf, 0, sd.count > 0 ? (long)sd.count : 0);
  const long first_nf = (R.nf == 1 && !meas_finite(y.raw(0))) ? 0 : sc.first_nf;
  return sd.count > 0 ? fmeas_found(sd, sc.hit, sc.khit, first_nf, R.nf) : fmeas_found(sd, sc.last, sc.klast, first_nf, R.nf);
}
// WHEN and FIND_WHEN from the search's record: value, status and d/dp_k into sens[k * stride] (sens may be null).  k2: the wrap count
// of s2 at the event's upper row (FIND_WHEN).
//   d u*/dp = (dL/dp - g_s(u*)) / g'(u*);  d f*/dp = ln 10 f* d u*/dp under LOG;  FIND_WHEN: g2_s(u*) + g2'(u*) d u*/dp
CH_MEAS_HD int fmeas_finish_event(const FRows& R, const ch_fmeasure_spec& sp, long s, const FLevel& lv, FFound f, long k2, double* value, double* sens, long stride) { CH_MEAS_NOCONTRACT
  const int np = (sens && R.dH) ? R.n_par : 0;
  const double* u = R.u(sp.xscale);
  const FSig y1 = fmeas_signal(R, sp.s1, s), y2 = fmeas_signal(R, sp.s2, s);
  int st = MEAS_OK;
  if (lv.bad || f.nonfinite) st = MEAS_NONFINITE;
  else if (f.i < 0) st = MEAS_NOT_FOUND;
  FAt p; double slope = 0.0, slope2 = 0.0, fstar = 0.0, v = 0.0;
  if (st == MEAS_OK) {
    const double r0 = y1.raw(f.i - 1), r1 = y1.raw(f.i);
    const double g0 = y1.val(r0, f.k - y1.wrap(r0, r1)), g1 = y1.val(r1, f.k);
    const double ux = fmeas_event_u(u, f.i, g0, g1, lv.L);
    fstar = fmeas_event_f(R, sp.xscale, f.i, g0, g1, lv.L);
    fmeas_weights(u, f.i, ux, p);
    slope = (g1 - g0) / (u[f.i] - u[f.i - 1]);
    v = fstar;
    if (sp.kind == CH_FMEAS_FIND_WHEN) {
      bool ok;
      v = fmeas_val_at(y2, p, k2, ok);
      slope2 = fmeas_slope_at(y2, u, p, k2);
      if (!ok) st = MEAS_NONFINITE;
    }
  }
  if (st != MEAS_OK) {
    *value = meas_nan();
    for (int k = 0; k < np; ++k) sens[k * stride] = meas_nan();
    return st;
  }
  if (!(slope != 0.0 && meas_finite(slope))) st = MEAS_FLAT;
  *value = v;
  for (int k = 0; k < np; ++k) {
    double d = meas_nan();
    if (st == MEAS_OK) {
      const FSig s1 = fmeas_sens_signal(R, sp.s1, s, k);
      const double dL = lv.rel ? fmeas_d_at(y1, s1, lv.p) : 0.0;
      const double du = (dL - fmeas_d_at(y1, s1, p)) / slope;
      if (sp.kind == CH_FMEAS_WHEN) d = sp.xscale == CH_FX_LOG ? 2.302585092994045684 * fstar * du : du;
      else d = fmeas_d_at(y2, fmeas_sens_signal(R, sp.s2, s, k), p) + slope2 * du;
    }
    sens[k * stride] = d;
  }
  return st;
}
// kat: the wrap count of the located place's upper row
CH_MEAS_HD void fmeas_find_at_locate(const FRows& R, const ch_fmeasure_spec& sp, FAt& p) { fmeas_locate(R.u(sp.xscale), R.nf, fmeas_u_of(sp.xscale, sp.at), p); }
CH_MEAS_HD int fmeas_find_at(const FRows& R, const ch_fmeasure_spec& sp, long s, const FAt& p, long kat, double* value, double* sens, long stride) {
  const int np = (sens && R.dH) ? R.n_par : 0;
  const FSig y = fmeas_signal(R, sp.s1, s);
  bool ok;
  const double v = fmeas_val_at(y, p, kat, ok);
  *value = ok ? v : meas_nan();
  for (int k = 0; k < np; ++k) sens[k * stride] = ok ? fmeas_d_at(y, fmeas_sens_signal(R, sp.s1, s, k), p) : meas_nan();
  return ok ? MEAS_OK : MEAS_NONFINITE;
}

// ---- windows ----
// [from, to] in Hz clipped to the grid.  The point set (from, the rows strictly inside, to) is walked interval by interval: interval i
// gives the piece [max(f_{i-1}, from), min(f_i, to)] with row values at rows and the line in (u, g) at from / to; the trapezoids are
// in linear f.  Keys order the points for "first occurrence": -1 the from point, i row i, nf the to point.
CH_MEAS_HD void fmeas_clip(const FRows& R, const ch_fmeasure_spec& sp, double& from, double& to) {
  from = sp.from > R.f[0] ? sp.from : R.f[0];
  to = sp.to < R.f[R.nf - 1] ? sp.to : R.f[R.nf - 1];
}
// intervals [ia, ib) into acc, k0 the wrap count of row ia - 1; sn: the sensitivity rows of one parameter (integ_s, ys), or null
CH_MEAS_HD void fmeas_window_chunk(const FRows& R, int xscale, const FSig& y, const FSig* sn, double from, double to, long ia, long ib, long k0, MeasAcc& acc) { CH_MEAS_NOCONTRACT
  if (ia >= ib) return;
  const double* u = R.u(xscale);
  double r0 = y.raw(ia - 1);
  long k = k0;
  for (long i = ia; i < ib; ++i) {
    const double r1 = y.raw(i);
    const long kprev = k;
    k += y.wrap(r0, r1);
    const double fa = R.f[i - 1], fb = R.f[i];
    const double g0 = y.val(r0, kprev), g1 = y.val(r1, k);
    r0 = r1;
    if (!(fb > from)) continue;
    if (!(fa < to)) break;
    const double s0 = sn ? y.d(*sn, i - 1) : 0.0, s1 = sn ? y.d(*sn, i) : 0.0;
    double xa = fa, xb = fb, ga = g0, gb = g1, sa = s0, sb = s1;
    if (from > fa) { FAt p; fmeas_weights(u, i, fmeas_u_of(xscale, from), p); xa = from; ga = p.w0 * g0 + p.w1 * g1; sa = p.w0 * s0 + p.w1 * s1; }
    if (to < fb) { FAt p; fmeas_weights(u, i, fmeas_u_of(xscale, to), p); xb = to; gb = p.w0 * g0 + p.w1 * g1; sb = p.w0 * s0 + p.w1 * s1; }
    if (!meas_finite(g0) || !meas_finite(g1) || !meas_finite(ga) || !meas_finite(gb)) acc.nonfinite = true;
    const double h = xb - xa;
    acc.integ += 0.5 * (ga + gb) * h; acc.sq += 0.5 * (ga * ga + gb * gb) * h;
    acc.integ_s += 0.5 * (sa + sb) * h; acc.ys += 0.5 * (ga * sa + gb * sb) * h;
    if (from >= fa) acc.point(ga, -1);
    acc.point(gb, to < fb ? R.nf : i);
  }
}
// d g / d p of one parameter at the point with this key: a row, or an end of a non-empty clipped window (`from` sits in the interval
// with f_{i-1} <= from < f_i, `to` in the one with f_{i-1} < to <= f_i; an end on a row's frequency is that row)
CH_MEAS_HD double fmeas_sens_at_key(const FRows& R, int xscale, const FSig& y, const FSig& sn, long key, double from, double to) {
  if (key >= 0 && key < R.nf) return y.d(sn, key);
  const bool is_from = key < 0;
  const double x = is_from ? from : to;
  long lo = 0, hi = R.nf - 1;
  while (hi - lo > 1) { const long mid = lo + (hi - lo) / 2; if (is_from ? R.f[mid] > x : R.f[mid] >= x) hi = mid; else lo = mid; }
  if (is_from && R.f[hi - 1] == x) return y.d(sn, hi - 1);
  if (!is_from && R.f[hi] == x) return y.d(sn, hi);
  FAt p;
  fmeas_weights(R.u(xscale), hi, fmeas_u_of(xscale, x), p);
  return fmeas_d_at(y, sn, p);
}
// a: the accumulation with parameter k's rows as sn
CH_MEAS_HD double fmeas_window_sens(int kind, const FRows& R, int xscale, const FSig& y, const FSig& sn, const MeasAcc& a, double from, double to) { CH_MEAS_NOCONTRACT
  switch (kind) {
    case CH_FMEAS_INTEG: return a.integ_s;
    case CH_FMEAS_AVG: return a.integ_s / (to - from);
    case CH_FMEAS_RMS: return a.ys / (std::sqrt(a.sq / (to - from)) * (to - from));
    case CH_FMEAS_MIN: return fmeas_sens_at_key(R, xscale, y, sn, a.kmn, from, to);
    case CH_FMEAS_MAX: return fmeas_sens_at_key(R, xscale, y, sn, a.kmx, from, to);
    default: return fmeas_sens_at_key(R, xscale, y, sn, a.kmx, from, to) - fmeas_sens_at_key(R, xscale, y, sn, a.kmn, from, to);
  }
}

// ---- one (measure, sample), the whole frequency axis in one pass: returns the status ----
CH_MEAS_HD int fmeas_eval(const FRows& R, const ch_fmeasure_spec& sp, long s, double* value, double* sens, long stride) {
  const FSig y = fmeas_signal(R, sp.s1, s);
  if (fmeas_is_event_kind(sp.kind)) {
    FLevel lv;
    fmeas_level_locate(R, sp.xscale, sp.s1, lv);
    fmeas_level_value(y, sp.s1, lv.rel ? y.kcount(1, lv.p.upper() + 1) : 0, lv);
    const FFound f = fmeas_search(R, sp.xscale, y, sp.s1, lv.L);
    const long k2 = (sp.kind == CH_FMEAS_FIND_WHEN && f.i >= 0) ? fmeas_signal(R, sp.s2, s).kcount(1, f.i + 1) : 0;
    return fmeas_finish_event(R, sp, s, lv, f, k2, value, sens, stride);
  }
  if (sp.kind == CH_FMEAS_FIND_AT) {
    FAt p;
    fmeas_find_at_locate(R, sp, p);
    return fmeas_find_at(R, sp, s, p, y.kcount(1, p.upper() + 1), value, sens, stride);
  }
  const int np = (sens && R.dH) ? R.n_par : 0;
  double from, to;
  fmeas_clip(R, sp, from, to);
  MeasAcc a; a.clear();
  fmeas_window_chunk(R, sp.xscale, y, nullptr, from, to, 1, R.nf, 0, a);
  const int st = meas_window_value(fmeas_window_kind(sp.kind), a, from, to, value);
  for (int k = 0; k < np; ++k) {
    if (st != MEAS_OK) { sens[k * stride] = meas_nan(); continue; }
    const FSig sn = fmeas_sens_signal(R, sp.s1, s, k);
    MeasAcc ak; ak.clear();
    fmeas_window_chunk(R, sp.xscale, y, &sn, from, to, 1, R.nf, 0, ak);
    sens[k * stride] = fmeas_window_sens(sp.kind, R, sp.xscale, y, sn, ak, from, to);
  }
  return st;
}

// ---- what the engine checks before anything is uploaded: null, or why the spec is refused ----
CH_MEAS_HD const char* fmeas_side_check(const ch_fmeasure_side& sd, int n_rows, int xscale, bool event) {
  if (sd.row_a < 0 || sd.row_a >= n_rows || sd.row_b < -1 || sd.row_b >= n_rows) return "a row out of range";
  if (sd.sig < 0 || sd.sig >= CH_FSIG_N) return "an unknown signal";
  if (!meas_finite(sd.scale)) return "a non-finite scale";
  if (!event) return nullptr;
  if (!meas_finite(sd.level)) return "a non-finite level";
  if (sd.count == 0 || sd.count < CH_MEAS_LAST) return "an event count of 0 (n >= 1, or CH_MEAS_LAST)";
  if (sd.edge < CH_EDGE_RISE || sd.edge > CH_EDGE_CROSS) return "an unknown edge";
  if (sd.fd != sd.fd) return "a NaN fd";
  if (xscale == CH_FX_LOG && meas_finite(sd.ref_at) && !(sd.ref_at > 0.0)) return "a reference frequency <= 0 on a LOG axis";
  return nullptr;
}
CH_MEAS_HD const char* fmeas_spec_check(const ch_fmeasure_spec& sp, int n_rows) {
  if (sp.kind < 0 || sp.kind >= CH_FMEAS_N_KINDS) return "an unknown kind";
  if (sp.xscale != CH_FX_LIN && sp.xscale != CH_FX_LOG) return "an unknown xscale";
  const char* why = fmeas_side_check(sp.s1, n_rows, sp.xscale, fmeas_is_event_kind(sp.kind));
  if (!why && fmeas_uses_s2(sp.kind)) why = fmeas_side_check(sp.s2, n_rows, sp.xscale, false);
  if (why) return why;
  if (sp.kind == CH_FMEAS_FIND_AT && sp.at != sp.at) return "a NaN frequency";
  if (sp.kind == CH_FMEAS_FIND_AT && sp.xscale == CH_FX_LOG && !(sp.at > 0.0)) return "a frequency <= 0 on a LOG axis";
  if (sp.kind >= CH_FMEAS_INTEG && (sp.from != sp.from || sp.to != sp.to)) return "a NaN window";
  return nullptr;
}
// the grid: null, or why it is refused
CH_MEAS_HD const char* fmeas_grid_check(const double* f, long nf, bool any_log) {
  for (long i = 0; i < nf; ++i) {
    if (!meas_finite(f[i]) || (i > 0 && !(f[i] > f[i - 1]))) return "frequencies must be finite and strictly increasing";
    if (any_log && !(f[i] > 0.0)) return "a LOG axis needs every frequency > 0";
  }
  return nullptr;
}

}  // namespace chip
