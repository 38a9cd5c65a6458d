// ch_noisesens_host.hpp — HIP-free half of the noise PSD parameter sensitivities (ch_noise_sens): the layout arithmetic of
// noisesens_solve_kernel (what stays resident, panel width, LDS and workspace sizes), the frequencies one launch of its
// 256-thread variant takes, and the MOSFET noise-parameter table with the extra row a perturbed instance column needs.
// Tested as a stand-alone program (tests/host_noisesens.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "ch_sens_host.hpp"   // dense_work_chunk, DENSE_WORK_CAP: the cap every 256-thread dense solver shares

namespace chip {

constexpr int NOISESENS_MAX_PANEL = 32;   // right-hand sides solved at once beside one factorisation

// doubles that stay resident for a whole system: the factors of Y^T and the adjoint solution y, a panel of one column (the layout
// is ch_sens_host.hpp's clu_*)
inline int noisesens_lda(int nc) { return clu_lda(nc); }
inline size_t noisesens_resident_doubles(int nc) { return clu_factor_doubles(nc) + clu_panel_doubles(nc, 1); }

// Parameter columns noisesens_solve_kernel<64> holds beside the resident part of an nc x nc system in `budget` doubles of dynamic
// LDS (a column is nc complex numbers): at most NOISESENS_MAX_PANEL and never more than n_par; 0 for n_par = 0 (the launch that
// only stores y).  -1: the resident part, or with n_par > 0 not even one column beside it, does not fit.
inline int noisesens_panel_columns(int nc, int n_par, size_t budget) {
  const size_t res = noisesens_resident_doubles(nc);
  if (nc < 1 || n_par < 0 || budget < res) return -1;
  if (n_par == 0) return 0;
  const size_t fit = (budget - res) / clu_panel_doubles(nc, 1);
  if (fit < 1) return -1;
  return (int)std::min<size_t>(std::min<size_t>(fit, NOISESENS_MAX_PANEL), (size_t)n_par);
}
// dynamic LDS of noisesens_solve_kernel<64> with panels of kp columns, in doubles
inline size_t noisesens_lds_doubles(int nc, int kp) { return noisesens_resident_doubles(nc) + clu_panel_doubles(nc, kp); }
// noisesens_solve_kernel<256>: panel width, and doubles of global workspace per system (resident part, one panel, the row
// permutation as ints packed two to a double)
inline int noisesens_work_columns(int n_par) { return std::min(std::max(n_par, 0), NOISESENS_MAX_PANEL); }
inline size_t noisesens_work_doubles(int nc, int kp) { return noisesens_lds_doubles(nc, kp) + clu_perm_doubles(nc); }
// frequencies one launch of the 256-thread variant takes: n_samples systems per frequency, under the cap of dense_work_chunk
inline int noisesens_freq_chunk(int nc, int kp, int n_samples, int n_freq) { return dense_work_chunk(noisesens_work_doubles(nc, kp), n_samples, n_freq); }

// The MOSFET noise-parameter table [n_cls][row] of an analysis in which one instance runs on a column of its own, class n_cls
// (perturb_tables, ch_param_tables.hpp): the same rows plus one more, a copy of the row of the class the instance belongs to.
// An empty result: cls_of_instance is no class of the table.
inline std::vector<double> noisesens_npar_extra_row(const std::vector<double>& table, int n_cls, int row, int cls_of_instance) {
  if (n_cls < 1 || row < 1 || cls_of_instance < 0 || cls_of_instance >= n_cls || table.size() < (size_t)n_cls * row) return std::vector<double>();
  std::vector<double> out(table.begin(), table.begin() + (size_t)n_cls * row);
  out.insert(out.end(), table.begin() + (size_t)cls_of_instance * row, table.begin() + (size_t)(cls_of_instance + 1) * row);
  return out;
}

}  // namespace chip
