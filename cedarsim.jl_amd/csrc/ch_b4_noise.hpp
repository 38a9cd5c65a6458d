// ch_b4_noise.hpp — BSIM4 MOSFET noise, the formula layer: operand row + noise parameters -> up to two (pwr, exponent) records
// between drain and source.  Host and device, nothing but <cmath>: tests/host_b4_noise.cpp runs it under ASan / UBSan against a
// long double restatement.  The operand row is filled on the device by b4_noise (ch_bsim4.hpp) from one evaluation of the core;
// the parameter row comes from ch_noise_params.hpp (card values, BSIM4.5 defaults where the card is silent).
//   record 0  channel thermal noise, tnoimod 0 (white):  4kT ntnoi ueff|qinv| / (leff^2 + ueff|qinv| rds)
//   record 1  flicker noise, exponent ef:  fnoimod 0  kf |ids|^af / (coxe leff^2);  fnoimod 1  the unified model of the BSIM4.5.0
//             manual, section 9.1, with lintnoi = 0
// tnoimod 1 (holistic thermal noise: a correlated source-side noise voltage) is refused by the host before any of this runs.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define CH_B4N_HD __host__ __device__ inline
#else
#define CH_B4N_HD inline
#endif

namespace chip {

// operand row of one instance at its operating point (mode frame)
enum B4NOp {
  B4NO_ids, B4NO_ueff, B4NO_vgsteff, B4NO_abulk, B4NO_vdseff, B4NO_vds, B4NO_rds, B4NO_esat, B4NO_litl, B4NO_leff, B4NO_weffnf,
  B4NO_coxe, B4NO_cdep0, B4NO_cit, B4NO_vtm, B4NO_qinv, B4NO_COUNT
};
// noise parameter row of one MOSFET class; the order of CH_B4N_* in include/cedarhip.h (ch_noise_params.hpp asserts it)
enum B4NPar {
  B4NP_noia, B4NP_noib, B4NP_noic, B4NP_em, B4NP_ef, B4NP_af, B4NP_kf, B4NP_ntnoi, B4NP_tnoia, B4NP_tnoib, B4NP_rnoia, B4NP_rnoib,
  B4NP_fnoimod, B4NP_tnoimod, B4NP_COUNT
};
struct B4NoiseRec {
  int a, b;        // terminal indices of the source in the device's own order (d, g, s, b): 0 and 2
  double pwr, ex;  // white: pwr [A^2/Hz]; flicker: pwr / f^ex
};
constexpr double B4N_KB = 1.380649e-23, B4N_Q = 1.60219e-19;   // k as the resistors' 4kT/R uses it; q as the model's packing does

// T in kelvin.  Returns the number of records written (always 2; a source that is off has pwr 0)
CH_B4N_HD int b4_noise_records(const double* op, const double* np, double T, B4NoiseRec* rec) {
  const double ids = std::fabs(op[B4NO_ids]), ueff = op[B4NO_ueff], leff = op[B4NO_leff], coxe = op[B4NO_coxe];
  const double l2 = leff * leff, kT = B4N_KB * T;
  // ---- channel thermal noise ----
  const double uq = ueff * std::fabs(op[B4NO_qinv]);
  rec[0].a = 0; rec[0].b = 2; rec[0].ex = 0.0;
  rec[0].pwr = 4.0 * kT * np[B4NP_ntnoi] * uq / (l2 + uq * op[B4NO_rds]);
  // ---- flicker noise ----
  rec[1].a = 0; rec[1].b = 2; rec[1].ex = np[B4NP_ef];
  if ((int)np[B4NP_fnoimod] == 0) {
    const double kf = np[B4NP_kf];
    rec[1].pwr = kf == 0.0 ? 0.0 : kf * std::pow(ids, np[B4NP_af]) / (coxe * l2);
    return 2;
  }
  if (ids == 0.0) { rec[1].pwr = 0.0; return 2; }
  const double vgst = op[B4NO_vgsteff], abulk = op[B4NO_abulk], vdseff = op[B4NO_vdseff], vtm = op[B4NO_vtm], litl = op[B4NO_litl];
  const double weffnf = op[B4NO_weffnf], noia = np[B4NP_noia], noib = np[B4NP_noib], noic = np[B4NP_noic];
  // N0 - Nl is formed from its own factor and the logarithm as log1p of it: near vds = 0, and at a very small vgsteff, the
  // differences of the textbook form cancel to nothing
  const double x = abulk * vdseff / (vgst + 2.0 * vtm);
  const double N0 = coxe * vgst / B4N_Q, Nl = N0 * (1.0 - x), dN = N0 * x;
  const double Ns = vtm * (coxe + op[B4NO_cdep0] + op[B4NO_cit]) / B4N_Q;
  double dl = litl * std::log(((op[B4NO_vds] - vdseff) / litl + np[B4NP_em]) / op[B4NO_esat]);
  if (!(dl > 0.0)) dl = 0.0;
  const double t_inv = kT * B4N_Q * B4N_Q * ueff * ids / (coxe * l2 * abulk * 1.0e10);
  const double br = noia * std::log1p(dN / (Nl + Ns)) + noib * dN + 0.5 * noic * dN * (N0 + Nl);
  const double t_clm = kT * ids * ids * dl / (weffnf * l2 * 1.0e10);
  const double s_inv = t_inv * br + t_clm * (noia + noib * Nl + noic * Nl * Nl) / ((Nl + Ns) * (Nl + Ns));
  const double s_wi = noia * kT * ids * ids / (weffnf * leff * Ns * Ns * 1.0e10);
  const double den = s_inv + s_wi;
  rec[1].pwr = den > 0.0 ? s_inv * s_wi / den : 0.0;
  return 2;
}

}  // namespace chip
