// ch_sens_host.hpp — HIP-free half of the DC parameter sensitivities (ch_dc_sens): the finite-difference step rule for
// dF/dp per slot kind and the step plan of a whole call (SensPlan: every sensitivity driver takes slot kinds, steps, divisors and
// perturbed values from it), the expansion of a solution in unknown order to MNA order, the layout arithmetic of sens_block_kernel
// and the workspace cap and chunk rule all three dense solvers share.  Tested as a stand-alone program (tests/host_sens_steps.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/cedarhip.h"
#include "ch_analysis.hpp"

namespace chip {

// How dF/dp_k is formed from residual evaluations at the fixed operating point:
//   forward: (F(p + h) - F(p)) / h with an ABSOLUTE step, for slots the residual is linear in — exact up to rounding whatever p is,
//            p = 0 included (a relative step of a tiny p, gmin = 1e-12 say, would put F(p + h) - F(p - h) below the rounding of F);
//   central: (F(p + h) - F(p - h)) / (2h) with h = rel_step * |p| (h = rel_step at p = 0) for everything else.
struct SensStep { bool central; double h; };

constexpr double SENS_REL_STEP = 1.0 / 131072.0;       // 2^-17
constexpr double SENS_GMIN_STEP = 1.0 / 1048576.0;     // 2^-20 S

// slot_kind: CH_SLOT_*; dev_kind: CH_DEV_* of the device a CH_SLOT_DEV_PAR slot addresses (0 otherwise); has_va: the circuit holds a
// compiled Verilog-A instance (a module may use $simparam("gmin") non-linearly); src_nonlinear: the slot's source sets the voltage
// of a known (eliminated) node that a MOSFET or compiled device sits on — the source then reaches the residual through that
// device's equations, not through a linear branch row (sens_sources_feeding_nonlinear); abs_step > 0 replaces the step, the kind
// of difference stays the slot's.
inline SensStep sens_step(int slot_kind, int dev_kind, bool has_va, bool src_nonlinear, double p, double rel_step, double abs_step) {
  bool linear = false; double h = 1.0;
  switch (slot_kind) {
    case CH_SLOT_SRC_DC: case CH_SLOT_SRC_PAR: linear = !src_nonlinear; break;
    case CH_SLOT_DEV_MULT: linear = true; break;
    case CH_SLOT_GMIN: linear = !has_va; h = SENS_GMIN_STEP; break;
    case CH_SLOT_DEV_PAR: linear = dev_kind == CH_DEV_VCVS || dev_kind == CH_DEV_VCCS; break;
    default: break;
  }
  if (abs_step > 0.0) return {!linear, abs_step};   // the caller's step; the kind of difference stays the slot's
  if (linear) return {false, h};
  const double r = rel_step > 0.0 ? rel_step : SENS_REL_STEP;
  return {true, p == 0.0 || !std::isfinite(p) ? r : r * std::fabs(p)};
}

// per source: 1 when it enters the known-value expression of a node that a nonlinear device (MOSFET, compiled Verilog-A) touches
inline std::vector<char> sens_sources_feeding_nonlinear(const Analysis& A, int n_src) {
  std::vector<char> nl(std::max(0, n_src), 0);
  for (const EDev& e : A.edev) {
    if (e.kind != K_MOS && e.kind != K_VA) continue;
    for (int k = 0; k < (e.kind == K_VA ? e.nt : 4); ++k) {
      if (e.term[k] >= 0) continue;
      for (const auto& tm : A.known[-e.term[k] - 1].terms) if (tm.first >= 0 && tm.first < n_src) nl[tm.first] = 1;
    }
  }
  return nl;
}

// The finite-difference plan of one sensitivity call, shared by every driver (ch_dc_sens, ch_ac_sens, ch_noise_sens, ch_tran_sens):
// per parameter its slot and how it is differenced, per (parameter, sample) the base value, the step and the divisor.
struct SensPlan {
  int n_par = 0, S = 0;
  std::vector<int> slot, kind, central, src_of;   // central: the kind of difference is a property of the slot, not of the sample;
                                                  // src_of: the source a CH_SLOT_SRC_DC / CH_SLOT_SRC_PAR slot addresses, -1 for any other
  std::vector<double> p, h, den;                  // [n_par][S]: the slot's value, the step, the divisor (2h central, h forward)
  bool is_src(int k) const { return src_of[k] >= 0; }
  // the slot's value in every sample for the evaluation of `sign` (+1, or -1 of a central difference): p + sign h
  std::vector<double> values(int k, int sign) const {
    std::vector<double> v(S);
    for (int s = 0; s < S; ++s) v[s] = p[(size_t)k * S + s] + sign * h[(size_t)k * S + s];
    return v;
  }
};

// slot_kind, slot_a, dev: the slot tables and the device list of the description; n_src: its sources; value(id, s): the value of slot
// id in sample s; opt: rel_step and, when given, abs_step[n_par]
template <class Value>
inline SensPlan sens_plan(const std::vector<int>& slot_kind, const std::vector<int>& slot_a, const std::vector<HDev>& dev, const Analysis& A, int n_src, int n_par,
                          const int32_t* slot_ids, int S, Value&& value, const ch_sens_opts& opt) {
  SensPlan P;
  P.n_par = n_par; P.S = S;
  P.slot.assign(slot_ids, slot_ids + n_par); P.kind.assign(n_par, 0); P.central.assign(n_par, 0); P.src_of.assign(n_par, -1);
  P.p.assign((size_t)n_par * S, 0.0); P.h.assign((size_t)n_par * S, 0.0); P.den.assign((size_t)n_par * S, 0.0);
  const std::vector<char> src_nl = sens_sources_feeding_nonlinear(A, n_src);
  for (int k = 0; k < n_par; ++k) {
    const int id = slot_ids[k], kind = slot_kind[id], sa = slot_a[id];
    const int dkind = kind == CH_SLOT_DEV_PAR ? dev[sa].kind : 0;
    const bool is_src = kind == CH_SLOT_SRC_DC || kind == CH_SLOT_SRC_PAR;
    P.kind[k] = kind; P.src_of[k] = is_src ? sa : -1;
    for (int s = 0; s < S; ++s) {
      const size_t at = (size_t)k * S + s;
      P.p[at] = value(id, s);
      const SensStep st = sens_step(kind, dkind, A.wide, is_src && src_nl[sa], P.p[at], opt.rel_step, opt.abs_step ? opt.abs_step[k] : 0.0);
      if (s == 0) P.central[k] = st.central ? 1 : 0;
      P.h[at] = st.h; P.den[at] = P.central[k] ? 2.0 * st.h : st.h;
    }
  }
  return P;
}

// d(known value)/dp of known node `k` for a slot that changes source `src` by dsrc per unit of p: the coefficient sum
inline double sens_known_deriv(const KnownDef& k, int src, double dsrc) {
  double s = 0.0;
  for (const auto& tm : k.terms) if (tm.first == src) s += tm.second;
  return s * dsrc;
}

// One sensitivity column in unknown order -> MNA order (the conventions of ch_dc): an unknown node (a node merged by a 0 V ammeter
// has its representative's unknown) takes its row, a known node the derivative of its known-value expression (src < 0: the slot is
// not a source slot, 0), an eliminated branch current is NaN.  su == nullptr: the operating point failed, unknown rows are NaN.
inline void sens_expand_mna(const Analysis& A, const double* su, int src, double dsrc, double* out) {
  for (int n = 1; n <= A.n_nodes; ++n) {
    const int u = A.node_unknown[n];
    if (u >= 0) out[n - 1] = su ? su[u] : CH_NAN;
    else out[n - 1] = src >= 0 ? sens_known_deriv(A.known[A.node_known[n]], src, dsrc) : 0.0;
  }
  for (int b = 0; b < A.n_branch; ++b) { const int u = A.branch_unknown[b]; out[A.n_nodes + b] = (u >= 0 && su) ? su[u] : CH_NAN; }
}

// Right-hand-side columns one launch of sens_block_kernel<64> holds beside an nc x nc matrix in `budget` doubles of LDS; the row
// stride lda = (nc + Kc) | 1 is odd, so that a column walk (pivot search, multipliers) touches every LDS bank once
inline int sens_lds_columns(int nc, size_t budget) { return (int)(budget / (size_t)std::max(1, nc)) - nc - 1; }
inline int sens_lda(int nc, int kc) { return (nc + kc) | 1; }

// The 256-thread variants of the dense solvers (ac_block_kernel, sens_block_kernel, acsens_solve_kernel) work in a global workspace
// that one launch may fill up to this cap: 2^27 doubles, 1 GiB
constexpr size_t DENSE_WORK_CAP = (size_t)1 << 27;
// How many of `n` items (frequencies, blocks) one launch takes when an item holds `n_sys` systems of `per` doubles each: as many
// as stay under the cap, at least 1 (a single item above the cap is left to hipMalloc to refuse)
inline int dense_work_chunk(size_t per, int n_sys, int n) {
  const size_t item = std::max<size_t>(1, per) * (size_t)std::max(1, n_sys);
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n), DENSE_WORK_CAP / item));
}

// Layout of the in-place complex LU (clu_factor with `perm`, ch_dense_lu.hpp) that acsens_solve_kernel, noisesens_solve_kernel and
// loopgain_solve_kernel share, in doubles per system.  clu_lda: the row stride of the factors, odd, so that a walk down a column
// (pivot search, multipliers, substitution) touches every LDS bank once per half-wave; the factors are two planes (real, imaginary)
// of nc rows; a panel holds k right-hand sides of nc complex numbers; the 256-thread variants keep the row permutation in their
// workspace as ints packed two to a double (the 64-thread ones in static LDS).
inline int clu_lda(int nc) { return nc | 1; }
inline size_t clu_factor_doubles(int nc) { return (size_t)2 * nc * clu_lda(nc); }
inline size_t clu_panel_doubles(int nc, int k) { return (size_t)2 * nc * k; }
inline size_t clu_perm_doubles(int nc) { return ((size_t)nc + 1) / 2; }

// sens_block_kernel<256>: right-hand-side columns per launch (at most 32), doubles of workspace per block, and blocks per launch
inline int sens_work_columns(int n_par) { return std::min(n_par, 32); }
inline size_t sens_work_doubles(int nc, int kc) { return (size_t)nc * sens_lda(nc, kc); }
inline int sens_block_chunk(int nc, int kc, int nblk) { return dense_work_chunk(sens_work_doubles(nc, kc), 1, nblk); }
// sens_block_kernel<64>: columns per launch, at least 1, in 2*96*97 doubles of LDS: the ceiling ch_create raises for ac_block_kernel<64> as well
inline int sens_lds_chunk_columns(int nc) { return std::max(1, sens_lds_columns(nc, (size_t)2 * 96 * 97)); }

}  // namespace chip
