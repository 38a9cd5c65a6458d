// ch_transens_host.hpp — HIP-free half of the transient parameter sensitivities (ch_tran_sens, direct method on the host stepper's
// accepted steps): the layout of the S / W rings and of the saved rows, the column-chunk rule of transens_step_kernel, the test
// that refuses a slot which moves a break point, the derivative of a known node's value at a time, and a scalar restatement of one
// step of the recursion for a dense block.  Tested as a stand-alone program (tests/host_transens.cpp).
//
// The recursion.  An accepted step to t_{n+1} solved f(x, t, p) + a0 q(x, p) + sum_j a_j q_j = 0 (a: bdf_coeffs, q_j: the Q ring).
// With the step sequence held fixed, s_k = dx_{n+1}/dp_k and w_{j,k} = dq_j/dp_k obey
//     (G + a0 C) s_k = -[ df/dp_k + a0 dq/dp_k + sum_j a_j w_{j,k} ],      w_{n+1,k} = C s_k + dq/dp_k
// with G, C and the partials at the accepted state.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "ch_sens_host.hpp"
#include "ch_stepper_host.hpp"

namespace chip {

// ---- rings S and W: [NSLOT][n_par][S][n_unk], indexed by the slot numbers StepControl hands out ----
inline size_t transens_ring_doubles(int n_par, int S, int n_unk) { return (size_t)NSLOT * n_par * S * n_unk; }
inline size_t transens_ring_index(int slot, int k, int s, int u, int n_par, int S, int n_unk) { return (((size_t)slot * n_par + k) * S + s) * n_unk + u; }
// a saved row of sensitivities: [n_obs][n_par][S]
inline size_t transens_row_doubles(int n_obs, int n_par, int S) { return (size_t)n_obs * n_par * S; }
// the perturbed dumps of one launch: column k of F+ / F- / Q+ / Q- starts k * f_stride doubles in, f_stride = nblk * ds
inline size_t transens_dump_index(int k, int blk, int i, int nblk, int ds) { return ((size_t)k * nblk + blk) * ds + i; }

// ---- column chunks ----
// transens_step_kernel<64> keeps [G + a0 C | b_0 .. b_{Kc-1}] in LDS with the odd row stride of sens_block_kernel; C streams from the
// global dump, so the column capacity is that of sens_block_kernel<64>.  Above 96 unknowns the 256-thread variant takes at most 32.
inline int transens_chunk_columns(int nc) { return nc <= 96 ? sens_lds_chunk_columns(nc) : 32; }
inline int transens_n_chunks(int nc, int n_par) { const int kc = transens_chunk_columns(nc); return (n_par + kc - 1) / kc; }
inline size_t transens_lds_doubles(int nc, int kc) { return (size_t)nc * sens_lda(nc, kc); }

// ---- a slot that moves a break point is not differentiable on a frozen step sequence ----
// true when the break-point times of the perturbed source parameters differ from those of the circuit's own (td, tr, pw, period of
// a PULSE; amplitudes, offsets and a SIN's frequency leave them alone).  The codes (jump or corner) are not compared: they steer the
// restart policy of a run whose steps are held fixed here anyway.
inline bool transens_moves_breakpoints(const std::vector<HSource>& srcs, const std::vector<double>& own_par, const std::vector<double>& pert_par, int n_sets,
                                       double t0, double t1) {
  std::vector<double> b0, c0, b1, c1;
  collect_breakpoints(srcs, own_par, n_sets, t0, t1, b0, c0);
  collect_breakpoints(srcs, pert_par, n_sets, t0, t1, b1, c1);
  return b0 != b1;
}

// ---- known nodes ----
// d(value of known node `k`)/dp at time t for a slot on source `src` (CH_SLOT_SRC_DC / CH_SLOT_SRC_PAR; src < 0: any other slot, 0):
// the coefficient sum of the source in the node's value expression times a forward difference of source_value at t, step h, between
// the perturbed tables (par_p, dc_p) and the circuit's own (par_0, dc_0).  is_value: the slot IS the source's value (exactly 1).
inline double transens_known_deriv(const KnownDef& k, const std::vector<HSource>& srcs, int src, bool is_value, const double* par_p, double dc_p,
                                   const double* par_0, double dc_0, double h, double t, int mode) {
  if (src < 0) return 0.0;
  if (is_value) return sens_known_deriv(k, src, 1.0);
  const double vp = source_value(srcs[src], par_p, dc_p, t, mode), v0 = source_value(srcs[src], par_0, dc_0, t, mode);
  return sens_known_deriv(k, src, (vp - v0) / h);
}

// ---- one step of the recursion for one dense block and one parameter, in plain scalar code ----
// G, C: n x n row-major; df, dq: the partials; alpha[0..k]; w_hist[j]: the n-vector w_{j} of history point j (j = 1..k at
// w_hist[j - 1]).  Gaussian elimination with partial pivoting (largest magnitude, lowest row on ties: the rule of the kernels).
// Returns false when G + a0 C does not factor.
inline bool transens_step_scalar(int n, const double* G, const double* C, const double* df, const double* dq, const double* alpha, int k,
                                 const double* const* w_hist, double* s_out, double* w_out) {
  std::vector<double> A((size_t)n * (n + 1));
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < n; ++j) A[(size_t)i * (n + 1) + j] = G[(size_t)i * n + j] + alpha[0] * C[(size_t)i * n + j];
    double h = 0.0;
    for (int m = 1; m <= k; ++m) h += alpha[m] * w_hist[m - 1][i];
    A[(size_t)i * (n + 1) + n] = -(df[i] + alpha[0] * dq[i] + h);
  }
  const int ld = n + 1;
  for (int c = 0; c < n; ++c) {
    int bi = c; double best = std::fabs(A[(size_t)c * ld + c]);
    for (int i = c + 1; i < n; ++i) if (std::fabs(A[(size_t)i * ld + c]) > best) { best = std::fabs(A[(size_t)i * ld + c]); bi = i; }
    if (!(best > 0.0) || !(best < 1e300)) return false;
    if (bi != c) for (int j = c; j <= n; ++j) std::swap(A[(size_t)c * ld + j], A[(size_t)bi * ld + j]);
    for (int i = c + 1; i < n; ++i) {
      const double l = A[(size_t)i * ld + c] / A[(size_t)c * ld + c];
      for (int j = c + 1; j <= n; ++j) A[(size_t)i * ld + j] -= l * A[(size_t)c * ld + j];
    }
  }
  for (int c = n - 1; c >= 0; --c) {
    double v = A[(size_t)c * ld + n];
    for (int j = c + 1; j < n; ++j) v -= A[(size_t)c * ld + j] * s_out[j];
    s_out[c] = v / A[(size_t)c * ld + c];
  }
  for (int i = 0; i < n; ++i) {
    double v = 0.0;
    for (int j = 0; j < n; ++j) v += C[(size_t)i * n + j] * s_out[j];
    w_out[i] = v + dq[i];
  }
  return true;
}

}  // namespace chip
