// ch_loopgain_host.hpp — HIP-free half of the loop-gain (stability) analysis, ch_loop_gain: the combination of the two probe responses
// into the loop gain and its derivative, the checks of the probe and of the slots, the entry of the current-injection right-hand side
// and the layout arithmetic of loopgain_solve_kernel.  DESIGN.md 2.7i has the definition in words.
//
// The probe is a voltage source x -> y in the loop wire.  Two excitations of Y(w) = G + jwC: the v-run (v_x - v_y = 1, keep V2 = v_x) and
// the i-run (probe at 0 V, unit current into node x, keep I1 = the probe's branch current, flowing from x through it to y).  Then
//   u = V2 - I1,   T = u / (1 - u),   dT/dp = (du/dp) / (1 - u)^2.
// The two functions of u run on the host and in the kernels (thread 0 of loopgain_solve_kernel, loopgain_dt_kernel).
// Tested as a stand-alone program (tests/host_loopgain.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "ch_measure_host.hpp"   // CH_MEAS_HD, CH_MEAS_NOCONTRACT
#include "ch_analysis.hpp"
#include "ch_sens_host.hpp"      // clu_*: the layout of the in-place complex LU

namespace chip {

// T = u / (1 - u).  1 - u = 0 is no failure: the division gives what IEEE gives (NaN or an infinity).
CH_MEAS_HD void loopgain_T_of_u(double ur, double ui, double& tr, double& ti) { CH_MEAS_NOCONTRACT
  const double dr = 1.0 - ur, di = -ui, den = dr * dr + di * di;
  tr = (ur * dr + ui * di) / den; ti = (ui * dr - ur * di) / den;
}
// dT = du / (1 - u)^2
CH_MEAS_HD void loopgain_dT_of_du(double ur, double ui, double dur, double dui, double& dtr, double& dti) { CH_MEAS_NOCONTRACT
  const double dr = 1.0 - ur, di = -ui, qr = dr * dr - di * di, qi = 2.0 * dr * di, den = qr * qr + qi * qi;
  dtr = (dur * qr + dui * qi) / den; dti = (dui * qr - dur * qi) / den;
}

// The i-run's right-hand side b_i: what `I 0 x ac=1` leaves in the engine's b = -(F(src + ac) - F(src)).  A current source p -> q with
// value i stamps F[p] += i, F[q] -= i (current leaving the node counts positive), so the terminal the current is driven INTO, the
// second one, gets b = +1 and the first one -1.
inline double loopgain_bi_entry(int terminal) { return terminal == 0 ? -1.0 : 1.0; }
constexpr int LOOPGAIN_BI_TERMINAL = 1;   // node x is the second terminal of `I 0 x`

// The probe as the solve sees it: the unknowns of v_x and of the branch current (global unknown indices)
struct LoopGainProbe { int u_x = -1, u_ip = -1; };

// null, or why device `probe_dev` cannot be the probe.  dev, src, A: the description's devices and sources and its analysis.
inline const char* loopgain_probe_check(const std::vector<HDev>& dev, const std::vector<HSource>& src, const Analysis& A, int probe_dev, LoopGainProbe& P) {
  P = LoopGainProbe();
  if (probe_dev < 0 || probe_dev >= (int)dev.size()) return "no such device";
  const HDev& d = dev[probe_dev];
  if (d.kind != CH_DEV_V) return "is not a voltage source";
  const int x = d.node[0];
  if (x <= 0 || x > A.n_nodes || A.node_unknown[x] < 0) return "its + node is ground or a node held by ideal sources (the loop signal must arrive at an unknown node)";
  if (d.branch < 0 || d.branch >= A.n_branch || d.eliminated || A.branch_unknown[d.branch] < 0)
    return "its branch current was eliminated (the probe must reach the engine as an AC-driven source: |ac| = 1)";
  const int si = d.ipar[0];
  if (si < 0 || si >= (int)src.size() || src[si].ac != 1.0) return "its source must carry |ac| = 1";
  for (int k = 0; k < (int)src.size(); ++k) if (k != si && src[k].ac != 0.0) return "another source carries an AC magnitude (every other AC excitation must be off)";
  P.u_x = A.node_unknown[x]; P.u_ip = A.branch_unknown[d.branch];
  return nullptr;
}

// true when slot `id` would move a right-hand side of the two runs: the probe's own multiplier (it scales the branch current the i-run
// reads against the unit current that is injected)
inline bool loopgain_slot_moves_b(const std::vector<int>& slot_kind, const std::vector<int>& slot_a, int id, int probe_dev) {
  return slot_kind[id] == CH_SLOT_DEV_MULT && slot_a[id] == probe_dev;
}

// ---- layout of loopgain_solve_kernel: the complex factors and a panel of two right-hand sides; the 256-thread variant adds the row
// permutation (the frequencies one of its launches takes: dense_work_chunk over n_samples systems of loopgain_work_doubles, through
// launch_freq_chunks) ----
inline int loopgain_lda(int nc) { return clu_lda(nc); }
inline size_t loopgain_lds_doubles(int nc) { return clu_factor_doubles(nc) + clu_panel_doubles(nc, 2); }
inline size_t loopgain_work_doubles(int nc) { return loopgain_lds_doubles(nc) + clu_perm_doubles(nc); }

}  // namespace chip
