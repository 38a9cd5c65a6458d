// ch_fmeasure_kernels.hpp — device side of the frequency-domain measurements (ch_freq_measure_rows, ch_ac_measure): a gather of the
// MNA rows the specs name out of the AC solve's device results, and two forms of the arithmetic of ch_fmeasure_host.hpp over rows
// [row][(par)][freq][sample] complex, samples fastest.
//   fmeasure_gather_kernel  x[S][n_freq][n_unk][2] (and z[S][n_freq][n_par][n_unk][2]) -> the compact rows; a known node is 0, a merged
//                           node reads its representative's unknown, an eliminated branch current and a skipped sample are NaN
//   fmeasure_lanes_kernel   a lane owns one (measure, sample) and walks the frequency axis (fmeas_eval as it stands); the 64 lanes of a
//                           wavefront are 64 consecutive samples.  The Monte-Carlo shape.
//   fmeasure_wave_kernel    a wavefront owns one (measure, sample); its lanes take 64 contiguous chunks of the intervals.  Event
//                           counts and the integer wrap counts k of the unwrapped phase go through wave prefix sums; window sums and
//                           extrema combine in the fixed butterfly of meas_wave_acc; lane 0 finishes with the other form's functions.
// Event frequencies, FIND_*, MIN / MAX and the unwrapped phase are bit-equal between the forms; the window sums differ in the order of
// their additions.  No LDS.  Included by ch_engine.hip behind every device header but ch_loopgain_kernels.hpp: the kernels in front keep their place in the
// code object.
#pragma once

#include "ch_fmeasure_host.hpp"
#include "ch_measure_kernels.hpp"

namespace chip {

struct FMeasureArgs {
  FRows rows;                      // H and dH point at the first sample of this launch
  const ch_fmeasure_spec* specs;   // rows already mapped to the rows of `rows`
  int n_meas, n_samples;           // samples of this launch
  double* value; int* status;      // [n_meas][ldo] at the first sample of this launch
  double* sens;                    // [n_meas][n_par][ldo], or null
  long ldo;
  const int* skip;                 // per sample of this launch: no operating point (status 5, NaN), or null
};

struct FGatherArgs {
  const double* x; const double* z;   // [S][n_freq][n_unk][2]; [S][n_freq][n_par][n_unk][2] or null
  const int* src; int n_used;         // per compact row: the unknown (>= 0), -1 a known node (0), -2 an eliminated branch current (NaN)
  const int* skip;                    // [S] or null
  int S, n_freq, n_unk, n_par;
  double* H; double* dH;              // [n_used][n_freq][S][2]; [n_used][n_par][n_freq][S][2]
};
// grid (ceil(S / 64), n_freq, n_used): one lane per sample, so the stores are contiguous (the loads stride by the system's size)
__global__ __launch_bounds__(64) void fmeasure_gather_kernel(const FGatherArgs a) {
  const long s = (long)blockIdx.x * 64 + threadIdx.x;
  const int f = blockIdx.y, r = blockIdx.z;
  if (s >= a.S) return;
  const int u = a.src[r];
  const bool nan = u == -2 || (a.skip && a.skip[s] && u >= 0);
  const long sf = s * a.n_freq + f;
  double re = 0.0, im = 0.0;
  if (nan) re = im = meas_nan();
  else if (u >= 0) { re = a.x[(sf * a.n_unk + u) * 2]; im = a.x[(sf * a.n_unk + u) * 2 + 1]; }
  const long o = (((long)r * a.n_freq + f) * a.S + s) * 2;
  a.H[o] = re; a.H[o + 1] = im;
  for (int k = 0; k < a.n_par; ++k) {
    double dre = 0.0, dim = 0.0;
    if (nan) dre = dim = meas_nan();
    else if (u >= 0) { dre = a.z[((sf * a.n_par + k) * a.n_unk + u) * 2]; dim = a.z[((sf * a.n_par + k) * a.n_unk + u) * 2 + 1]; }
    const long od = ((((long)r * a.n_par + k) * a.n_freq + f) * a.S + s) * 2;
    a.dH[od] = dre; a.dH[od + 1] = dim;
  }
}

__device__ inline void fmeas_no_op(const FMeasureArgs& a, int mi, long s) {
  a.value[(long)mi * a.ldo + s] = meas_nan();
  a.status[(long)mi * a.ldo + s] = FMEAS_NO_OP;
  if (a.sens) for (int k = 0; k < a.rows.n_par; ++k) a.sens[((long)mi * a.rows.n_par + k) * a.ldo + s] = meas_nan();
}

__global__ __launch_bounds__(64) void fmeasure_lanes_kernel(const FMeasureArgs a) {
  const long s = (long)blockIdx.x * 64 + threadIdx.x;
  const int mi = blockIdx.y;
  if (s >= a.n_samples) return;
  if (a.skip && a.skip[s]) { fmeas_no_op(a, mi, s); return; }
  double v;
  double* sens = a.sens ? a.sens + (long)mi * a.rows.n_par * a.ldo + s : nullptr;
  const int st = fmeas_eval(a.rows, a.specs[mi], s, &v, sens, a.ldo);
  a.value[(long)mi * a.ldo + s] = v;
  a.status[(long)mi * a.ldo + s] = st;
}

__device__ inline long fmeas_wave_sum(long v) { for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
// exclusive prefix sum over the lanes
__device__ inline long fmeas_wave_excl(long v, int lane) {
  long incl = v;
  for (int d = 1; d < 64; d <<= 1) { const long o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
  return incl - v;
}
// the wrap count of row `row` (k_0 = 0): every lane counts the wraps of its own chunk up to that row; integers, so the sum is exact
__device__ inline long fmeas_wave_k_at(const FSig& y, long ia, long ib, long row) {
  if (y.sig != CH_FSIG_PHASE) return 0;
  return fmeas_wave_sum(y.kcount(ia, ib < row + 1 ? ib : row + 1));
}
// the event search of fmeas_search over 64 chunks: every lane returns the same record
__device__ inline FFound fmeas_wave_search(const FRows& R, int xscale, const FSig& y, const ch_fmeasure_side& sd, double L, long ia, long ib, long k0, int lane) {
  const FScan sc = fmeas_scan(R, xscale, y, sd, L, ia, ib, k0, 0);
  long first_nf = meas_wave_min(sc.first_nf);
  if (R.nf == 1 && !meas_finite(y.raw(0))) first_nf = 0;
  const long none = -0x7fffffffffffffffL;
  long found, kf;
  if (sd.count > 0) {
    const long excl = fmeas_wave_excl(sc.count, lane), incl = excl + sc.count;
    long hit = -1, khit = none;
    if (excl < sd.count && (long)sd.count <= incl) { const FScan h = fmeas_scan(R, xscale, y, sd, L, ia, ib, k0, (long)sd.count - excl); hit = h.hit; khit = h.khit; }   // at most one lane
    found = meas_wave_max(hit); kf = meas_wave_max(khit);
  } else {
    found = meas_wave_max(sc.last);
    kf = meas_wave_max((found >= 0 && sc.last == found) ? sc.klast : none);
  }
  return fmeas_found(sd, found, found >= 0 ? kf : 0, first_nf, R.nf);
}

__global__ __launch_bounds__(64) void fmeasure_wave_kernel(const FMeasureArgs a) {
  const int lane = threadIdx.x, mi = blockIdx.y;
  const long s = blockIdx.x;
  if (a.skip && a.skip[s]) { if (lane == 0) fmeas_no_op(a, mi, s); return; }
  const FRows& R = a.rows;
  const ch_fmeasure_spec sp = a.specs[mi];
  double* sens = a.sens ? a.sens + (long)mi * R.n_par * a.ldo + s : nullptr;
  const long out = (long)mi * a.ldo + s;
  const FSig y = fmeas_signal(R, sp.s1, s);
  long ia, ib;
  meas_lane_chunk(R.nf, lane, ia, ib);
  if (sp.kind == CH_FMEAS_FIND_AT) {
    FAt p;
    fmeas_find_at_locate(R, sp, p);
    const long kat = fmeas_wave_k_at(y, ia, ib, p.upper());
    if (lane == 0) { double v; a.status[out] = fmeas_find_at(R, sp, s, p, kat, &v, sens, a.ldo); a.value[out] = v; }
    return;
  }
  const long k0 = fmeas_wave_excl(y.kcount(ia, ib), lane);   // the wrap count of row ia - 1
  if (fmeas_is_event_kind(sp.kind)) {
    FLevel lv;
    fmeas_level_locate(R, sp.xscale, sp.s1, lv);
    fmeas_level_value(y, sp.s1, lv.rel ? fmeas_wave_k_at(y, ia, ib, lv.p.upper()) : 0, lv);
    const FFound f = fmeas_wave_search(R, sp.xscale, y, sp.s1, lv.L, ia, ib, k0, lane);
    const long k2 = (sp.kind == CH_FMEAS_FIND_WHEN && f.i >= 0) ? fmeas_wave_k_at(fmeas_signal(R, sp.s2, s), ia, ib, f.i) : 0;
    if (lane == 0) { double v; a.status[out] = fmeas_finish_event(R, sp, s, lv, f, k2, &v, sens, a.ldo); a.value[out] = v; }
    return;
  }
  const int np = (sens && R.dH) ? R.n_par : 0;
  double from, to;
  fmeas_clip(R, sp, from, to);
  MeasAcc acc; acc.clear();
  fmeas_window_chunk(R, sp.xscale, y, nullptr, from, to, ia, ib, k0, acc);
  acc = meas_wave_acc(acc, lane);
  int st = MEAS_OK;
  if (lane == 0) { double v; st = meas_window_value(fmeas_window_kind(sp.kind), acc, from, to, &v); a.status[out] = st; a.value[out] = v; }
  st = __shfl(st, 0, 64);
  for (int k = 0; k < np; ++k) {
    if (st != MEAS_OK) { if (lane == 0) sens[(long)k * a.ldo] = meas_nan(); continue; }
    const FSig sn = fmeas_sens_signal(R, sp.s1, s, k);
    MeasAcc ak; ak.clear();
    fmeas_window_chunk(R, sp.xscale, y, &sn, from, to, ia, ib, k0, ak);
    ak = meas_wave_acc(ak, lane);
    if (lane == 0) sens[(long)k * a.ldo] = fmeas_window_sens(sp.kind, R, sp.xscale, y, sn, ak, from, to);
  }
}

}  // namespace chip
