// ch_acsens_host.hpp — HIP-free half of the AC parameter sensitivities (ch_ac_sens): the layout arithmetic of acsens_solve_kernel
// (panel width, LDS and workspace size), the system size of ac_block_kernel, the step of the state term and the expansion of a
// complex row (ch_ac, ch_ac_sens) from unknown order to MNA order.  Tested as a stand-alone program (tests/host_acsens.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "../../include/cedarhip.h"
#include "ch_analysis.hpp"
#include "ch_sens_host.hpp"

namespace chip {

constexpr int ACSENS_MAX_PANEL = 32;   // right-hand sides solved at once beside one factorisation

// row stride and doubles of the complex factors of acsens_solve_kernel: the shared layout of ch_sens_host.hpp
inline int acsens_lda(int nc) { return clu_lda(nc); }
inline size_t acsens_factor_doubles(int nc) { return clu_factor_doubles(nc); }

// Right-hand-side columns acsens_solve_kernel<64> holds beside the factors of an nc x nc system in `budget` doubles of dynamic LDS
// (a column is nc complex numbers): at least 1 when the factors fit at all, at most ACSENS_MAX_PANEL and never more than n_par;
// 0 when not even one column fits
inline int acsens_panel_columns(int nc, int n_par, size_t budget) {
  const size_t fac = clu_factor_doubles(nc);
  if (nc < 1 || n_par < 1 || budget < fac + clu_panel_doubles(nc, 1)) return 0;
  const size_t fit = (budget - fac) / clu_panel_doubles(nc, 1);
  return (int)std::min<size_t>(std::min<size_t>(fit, ACSENS_MAX_PANEL), (size_t)n_par);
}

// acsens_solve_kernel: doubles of dynamic LDS (T = 64: factors and one panel of kc columns; the layout is ch_sens_host.hpp's clu_*)
// and of global workspace per system (T = 256: the row permutation as well); the frequencies one launch takes come from
// dense_work_chunk
inline size_t acsens_lds_doubles(int nc, int kc) { return clu_factor_doubles(nc) + clu_panel_doubles(nc, kc); }
inline size_t acsens_work_doubles(int nc, int kc) { return acsens_lds_doubles(nc, kc) + clu_perm_doubles(nc); }
// ac_block_kernel: doubles per system, in LDS (T = 64) or in the global workspace (T = 256): [G + jwC | b], row stride nc + 1
inline size_t ac_system_doubles(int nc) { return (size_t)2 * nc * (nc + 1); }

// Step of the state term for one (sample, parameter): G and C are differenced at x* +- eps * s, s = dx*/dp in unknown order, with
// eps such that the largest shift of a node-voltage unknown is dv (nonlinear devices are voltage-controlled; branch currents enter
// the residual linearly).  0 = the term is skipped: s is zero (or not finite) on every node unknown.
inline double acsens_state_eps(const Analysis& A, const double* s, double dv) {
  double m = 0.0;
  for (int n = 1; n <= A.n_nodes; ++n) {
    const int u = A.node_unknown[n];
    if (u < 0) continue;
    const double v = std::fabs(s[u]);
    if (!std::isfinite(v)) return 0.0;
    m = std::max(m, v);
  }
  if (!(m > 0.0)) return 0.0;
  const double eps = dv / m;
  return eps > 0.0 && std::isfinite(eps) ? eps : 0.0;
}

// true when G or C can depend on the state: the circuit holds a MOSFET or a compiled Verilog-A instance
inline bool acsens_state_dependent(const Analysis& A) {
  for (const EDev& e : A.edev) if (e.kind == K_MOS || e.kind == K_VA) return true;
  return false;
}

// One complex row (an AC solution or a sensitivity) in unknown order ([n_unk][2]) -> MNA order ([n_mna][2]): an unknown node (a
// node merged by a 0 V ammeter has its representative's unknown) takes its row, a known node carries no small signal (0: AC-driven
// sources are never eliminated), an eliminated branch current is NaN.  zu == nullptr: the sample was not served, unknown rows are NaN.
inline void acsens_expand_mna(const Analysis& A, const double* zu, double* out) {
  for (int n = 1; n <= A.n_nodes; ++n) {
    const int u = A.node_unknown[n];
    for (int c = 0; c < 2; ++c) out[2 * (n - 1) + c] = u >= 0 ? (zu ? zu[2 * u + c] : CH_NAN) : 0.0;
  }
  for (int b = 0; b < A.n_branch; ++b) {
    const int u = A.branch_unknown[b];
    for (int c = 0; c < 2; ++c) out[2 * (A.n_nodes + b) + c] = (u >= 0 && zu) ? zu[2 * u + c] : CH_NAN;
  }
}

}  // namespace chip
