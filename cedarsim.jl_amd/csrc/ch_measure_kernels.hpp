// ch_measure_kernels.hpp — device side of the waveform measurements (ch_measure_rows, ch_result_measure): two forms of the arithmetic
// of ch_measure_host.hpp over rows [row][time][sample], samples fastest.
//   measure_lanes_kernel  a lane owns one (measure, sample) and walks the time axis (meas_eval as it stands); the 64 lanes of a
//                         wavefront are 64 consecutive samples, so every load along the sample axis is contiguous.  The Monte-Carlo shape.
//   measure_wave_kernel   a wavefront owns one (measure, sample); its lanes take 64 contiguous chunks of the intervals.  Event counts
//                         go through a wave prefix sum and the lane that holds the wanted event finds it; window sums and extrema
//                         combine in a fixed butterfly order.  One circuit with a long waveform.
// Event times, FIND_* and MIN / MAX come out of the same functions with the same arguments in both forms (bit-equal); the window sums
// differ in the order of their additions.  No LDS; no kernel in front of these is touched.
// Included by ch_engine.hip behind ch_transens_kernels.hpp: the kernels in front of it keep their place in the code object.
#pragma once

#include "ch_measure_host.hpp"

namespace chip {

struct MeasureArgs {
  MeasRows rows;                  // V and Sn point at the first sample of this launch
  const ch_measure_spec* specs;   // rows already mapped to the rows of `rows`
  int n_meas, n_samples;          // samples of this launch
  double* value; int* status;     // [n_meas][ldo] at the first sample of this launch
  double* sens;                   // [n_meas][n_par][ldo], or null
  long ldo;
};

__global__ __launch_bounds__(64) void measure_lanes_kernel(const MeasureArgs a) {
  const long s = (long)blockIdx.x * 64 + threadIdx.x;
  const int mi = blockIdx.y;
  if (s >= a.n_samples) return;
  double v;
  double* sens = a.sens ? a.sens + (long)mi * a.rows.n_par * a.ldo + s : nullptr;
  const int st = meas_eval(a.rows, a.specs[mi], s, &v, sens, a.ldo);
  a.value[(long)mi * a.ldo + s] = v;
  a.status[(long)mi * a.ldo + s] = st;
}

__device__ inline long meas_wave_max(long v) { for (int d = 32; d >= 1; d >>= 1) { const long o = __shfl_xor(v, d, 64); v = o > v ? o : v; } return v; }
__device__ inline long meas_wave_min(long v) { for (int d = 32; d >= 1; d >>= 1) { const long o = __shfl_xor(v, d, 64); v = o < v ? o : v; } return v; }
// the 64 chunk records into one, in a fixed order: after the step with distance d, every lane that is a multiple of 2 d holds its own
// 2 d chunks, the later half added to the earlier
__device__ inline MeasAcc meas_wave_acc(MeasAcc a, int lane) {
  for (int d = 1; d < 64; d <<= 1) {
    MeasAcc o;
    o.integ = __shfl_down(a.integ, d, 64); o.sq = __shfl_down(a.sq, d, 64); o.integ_s = __shfl_down(a.integ_s, d, 64); o.ys = __shfl_down(a.ys, d, 64);
    o.mn = __shfl_down(a.mn, d, 64); o.mx = __shfl_down(a.mx, d, 64); o.kmn = __shfl_down(a.kmn, d, 64); o.kmx = __shfl_down(a.kmx, d, 64);
    o.nonfinite = __shfl_down((int)a.nonfinite, d, 64) != 0;
    if ((lane & (2 * d - 1)) == 0) a.add(o);   // lanes 0, 2d, 4d, ...: their 2d chunks in time order
  }
  return a;   // complete in lane 0
}
// the event search of meas_search over 64 chunks: every lane returns the same record
__device__ inline MeasFound meas_wave_search(const MeasRows& R, const MeasSig& y, const ch_measure_side& sd, int lane) {
  long ia, ib;
  meas_lane_chunk(R.nt, lane, ia, ib);
  const MeasScan sc = meas_scan(R, y, sd, ia, ib, 0);
  long first_nf = meas_wave_min(sc.first_nf);
  if (R.nt == 1 && !meas_finite(y.at(0))) first_nf = 0;
  long found;
  if (sd.count > 0) {
    long incl = sc.count;   // inclusive prefix sum of the lanes' counts
    for (int d = 1; d < 64; d <<= 1) { const long o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
    const long excl = incl - sc.count;
    long hit = -1;
    if (excl < sd.count && (long)sd.count <= incl) hit = meas_scan(R, y, sd, ia, ib, (long)sd.count - excl).hit;   // at most one lane
    found = meas_wave_max(hit);
  } else found = meas_wave_max(sc.last);
  return meas_found(sd, found, first_nf, R.nt);
}

__global__ __launch_bounds__(64) void measure_wave_kernel(const MeasureArgs a) {
  const int lane = threadIdx.x, mi = blockIdx.y;
  const long s = blockIdx.x;
  const MeasRows& R = a.rows;
  const ch_measure_spec sp = a.specs[mi];
  double* sens = a.sens ? a.sens + (long)mi * R.n_par * a.ldo + s : nullptr;
  const long out = (long)mi * a.ldo + s;
  if (meas_is_event_kind(sp.kind)) {
    const MeasFound f1 = meas_wave_search(R, meas_signal(R, sp.s1, s), sp.s1, lane);
    MeasFound f2; f2.i = -1; f2.nonfinite = false;
    if (sp.kind == CH_MEAS_DELAY) f2 = meas_wave_search(R, meas_signal(R, sp.s2, s), sp.s2, lane);
    if (lane == 0) { double v; a.status[out] = meas_finish_event(R, sp, s, f1, f2, &v, sens, a.ldo); a.value[out] = v; }
    return;
  }
  if (sp.kind == CH_MEAS_FIND_AT) {
    if (lane == 0) { double v; a.status[out] = meas_find_at(R, sp, s, &v, sens, a.ldo); a.value[out] = v; }
    return;
  }
  const int np = (sens && R.Sn) ? R.n_par : 0;
  const MeasSig y = meas_signal(R, sp.s1, s);
  double from, to;
  meas_clip(R, sp, from, to);
  long ia, ib;
  meas_lane_chunk(R.nt, lane, ia, ib);
  MeasAcc acc; acc.clear();
  meas_window_chunk(R, y, nullptr, from, to, ia, ib, acc);
  acc = meas_wave_acc(acc, lane);
  int st = MEAS_OK;
  if (lane == 0) { double v; st = meas_window_value(sp.kind, acc, from, to, &v); a.status[out] = st; a.value[out] = v; }
  st = __shfl(st, 0, 64);
  for (int k = 0; k < np; ++k) {
    if (st != MEAS_OK) { if (lane == 0) sens[(long)k * a.ldo] = meas_nan(); continue; }
    const MeasSig sn = meas_sens_signal(R, sp.s1, s, k);
    MeasAcc ak; ak.clear();
    meas_window_chunk(R, y, &sn, from, to, ia, ib, ak);
    ak = meas_wave_acc(ak, lane);
    if (lane == 0) sens[(long)k * a.ldo] = meas_window_sens(sp.kind, R, sn, ak, from, to);
  }
}

}  // namespace chip
