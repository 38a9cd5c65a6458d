// ch_noise_params.hpp — the BSIM4 noise parameters on their own channel, HIP-free (tests/host_b4_noise.cpp runs it under ASan /
// UBSan).  The card vector of ch_desc.model_par and the packed column of the hot kernels do not carry them (the .def lists them as
// accepted and ignored); ch_set_mos_noise hands one row of CH_B4N_NPAR doubles per model, NaN = not given, and the noise analysis
// packs one row per MOSFET class: card value, else the BSIM4.5 default of the device type.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/cedarhip.h"
#include "ch_b4_noise.hpp"

namespace chip {

static_assert((int)CH_B4N_noia == (int)B4NP_noia && (int)CH_B4N_noib == (int)B4NP_noib && (int)CH_B4N_noic == (int)B4NP_noic && (int)CH_B4N_em == (int)B4NP_em &&
              (int)CH_B4N_ef == (int)B4NP_ef && (int)CH_B4N_af == (int)B4NP_af && (int)CH_B4N_kf == (int)B4NP_kf && (int)CH_B4N_ntnoi == (int)B4NP_ntnoi &&
              (int)CH_B4N_tnoia == (int)B4NP_tnoia && (int)CH_B4N_tnoib == (int)B4NP_tnoib && (int)CH_B4N_rnoia == (int)B4NP_rnoia && (int)CH_B4N_rnoib == (int)B4NP_rnoib &&
              (int)CH_B4N_fnoimod == (int)B4NP_fnoimod && (int)CH_B4N_tnoimod == (int)B4NP_tnoimod && (int)CH_B4N_NPAR == (int)B4NP_COUNT,
              "the formula layer and the C-ABI name the noise parameters in one order");
static_assert((int)CH_B4N_NOPERAND == (int)B4NO_COUNT, "the operand row of ch_noise_sources is the formula layer's");

// BSIM4.5 default of noise parameter i for a device of the given type (+1 n, -1 p)
inline double b4n_default(int i, double type) {
  const bool n = type > 0.0;
  switch (i) {
    case CH_B4N_noia: return n ? 6.25e41 : 6.188e40;
    case CH_B4N_noib: return n ? 3.125e26 : 1.5e25;
    case CH_B4N_noic: return 8.75e9;
    case CH_B4N_em: return 4.1e7;
    case CH_B4N_ef: return 1.0;
    case CH_B4N_af: return 1.0;
    case CH_B4N_kf: return 0.0;
    case CH_B4N_ntnoi: return 1.0;
    case CH_B4N_tnoia: return 1.5;
    case CH_B4N_tnoib: return 3.5;
    case CH_B4N_rnoia: return 0.577;
    case CH_B4N_rnoib: return 0.5164;
    case CH_B4N_fnoimod: return 1.0;
    case CH_B4N_tnoimod: return 0.0;
  }
  return 0.0;
}

// one packed row: `given` is the model's row as ch_set_mos_noise got it (NaN = not given), or null when it got none
inline void b4n_pack(const double* given, double type, double* row) {
  for (int i = 0; i < CH_B4N_NPAR; ++i) row[i] = (given && !std::isnan(given[i])) ? given[i] : b4n_default(i, type);
}

// What the one-port (pwr, exponent) table cannot express is refused; `what` names the selector
inline int b4n_check(const double* row, std::string& what) {
  if ((int)row[CH_B4N_tnoimod] != 0) { what = "tnoimod = " + std::to_string((int)row[CH_B4N_tnoimod]) + " (the holistic thermal noise model has a correlated source-side noise voltage)"; return CH_ERR_UNSUPPORTED; }
  const int fm = (int)row[CH_B4N_fnoimod];
  if (fm != 0 && fm != 1) { what = "fnoimod = " + std::to_string(fm); return CH_ERR_UNSUPPORTED; }
  return CH_OK;
}

// The table of one analysis: [n_cls][CH_B4N_NPAR], class cl of model model_of[cl] and type type_of[cl].  given[m] is empty or
// CH_B4N_NPAR long.  On a refusal `err` names the model card by its index in ch_desc.
inline int b4n_table(const std::vector<int>& model_of, const std::vector<double>& type_of, const std::vector<std::vector<double>>& given, std::vector<double>& table,
                     std::string& err) {
  const size_t n = model_of.size();
  table.assign(std::max<size_t>(1, n) * CH_B4N_NPAR, 0.0);
  for (size_t cl = 0; cl < n; ++cl) {
    const int m = model_of[cl];
    const double* g = (m >= 0 && (size_t)m < given.size() && given[m].size() == (size_t)CH_B4N_NPAR) ? given[m].data() : nullptr;
    double* row = table.data() + cl * CH_B4N_NPAR;
    b4n_pack(g, type_of[cl], row);
    std::string what;
    const int rc = b4n_check(row, what);
    // (the Python layer reads the index behind "model card " to add the card's name: NoiseSolution._failure, solution.py)
    if (rc != CH_OK) { err = "MOSFET noise: model card " + std::to_string(m) + " selects " + what + ", which the engine does not build"; return rc; }
  }
  return CH_OK;
}

}  // namespace chip
