// host_b4_noise.cpp — the formula layer of the BSIM4 MOSFET noise (ch_b4_noise.hpp: b4_noise_records) and the packing of its
// parameters (ch_noise_params.hpp) as a stand-alone program; tests/test_host_b4_noise.py builds it with ASan + UBSan.
// Every record is held to a long double restatement of the same formulas over a grid of operand rows.  The tolerance is measured
// here: the largest relative deviation from the long double value of a SECOND double evaluation that associates the same formulas
// differently, times 8, floored at 1e-14.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "ch_noise_params.hpp"

using namespace chip;
typedef long double LD;

static const LD KB = 1.380649e-23L, QE = 1.60219e-19L;

// the restatement: same formulas, long double throughout
static void ref_records(const double* op, const double* np, double T, LD* thermal, LD* flicker) {
  const LD ids = fabsl((LD)op[B4NO_ids]), ueff = op[B4NO_ueff], leff = op[B4NO_leff], coxe = op[B4NO_coxe], kT = KB * (LD)T;
  const LD uq = ueff * fabsl((LD)op[B4NO_qinv]);
  *thermal = 4.0L * kT * (LD)np[B4NP_ntnoi] * uq / (leff * leff + uq * (LD)op[B4NO_rds]);
  if ((int)np[B4NP_fnoimod] == 0) { *flicker = np[B4NP_kf] == 0.0 ? 0.0L : (LD)np[B4NP_kf] * powl(ids, (LD)np[B4NP_af]) / (coxe * leff * leff); return; }
  if (ids == 0.0L) { *flicker = 0.0L; return; }
  const LD vg = op[B4NO_vgsteff], ab = op[B4NO_abulk], vde = op[B4NO_vdseff], vtm = op[B4NO_vtm], litl = op[B4NO_litl], wn = op[B4NO_weffnf];
  const LD a = np[B4NP_noia], b = np[B4NP_noib], c = np[B4NP_noic];
  const LD x = ab * vde / (vg + 2.0L * vtm), N0 = coxe * vg / QE, Nl = N0 * (1.0L - x), dN = N0 * x, Ns = vtm * (coxe + (LD)op[B4NO_cdep0] + (LD)op[B4NO_cit]) / QE;
  LD dl = litl * logl((((LD)op[B4NO_vds] - vde) / litl + (LD)np[B4NP_em]) / (LD)op[B4NO_esat]);
  if (!(dl > 0.0L)) dl = 0.0L;
  const LD s_inv = kT * QE * QE * ueff * ids / (coxe * leff * leff * ab * 1.0e10L) * (a * log1pl(dN / (Nl + Ns)) + b * dN + 0.5L * c * dN * (N0 + Nl)) +
                   kT * ids * ids * dl / (wn * leff * leff * 1.0e10L) * (a + b * Nl + c * Nl * Nl) / ((Nl + Ns) * (Nl + Ns));
  const LD s_wi = a * kT * ids * ids / (wn * leff * Ns * Ns * 1.0e10L);
  *flicker = (s_inv + s_wi) > 0.0L ? s_inv * s_wi / (s_inv + s_wi) : 0.0L;
}

// the same formulas in double, associated differently: divisions turned into products of reciprocals, sums reordered, the harmonic
// mean as 1 / (1/a + 1/b), Nl as N0 - N0 x.  (All three form N0 - Nl = N0 x from its own factor and the logarithm as log1p of
// (N0 - Nl)/(Nl + N*), as the code does: the textbook differences cancel to nothing at a very small vgsteff, in long double too.)
static void alt_records(const double* op, const double* np, double T, double* thermal, double* flicker) {
  const double ids = std::fabs(op[B4NO_ids]), ueff = op[B4NO_ueff], leff = op[B4NO_leff], coxe = op[B4NO_coxe], kT = T * 1.380649e-23, q = 1.60219e-19;
  const double il2 = 1.0 / (leff * leff), uq = std::fabs(op[B4NO_qinv]) * ueff;
  *thermal = (kT * uq) * (np[B4NP_ntnoi] * 4.0) / (uq * op[B4NO_rds] + leff * leff);
  if ((int)np[B4NP_fnoimod] == 0) { *flicker = np[B4NP_kf] == 0.0 ? 0.0 : std::pow(ids, np[B4NP_af]) * il2 * (np[B4NP_kf] / coxe); return; }
  if (ids == 0.0) { *flicker = 0.0; return; }
  const double vg = op[B4NO_vgsteff], ab = op[B4NO_abulk], vde = op[B4NO_vdseff], vtm = op[B4NO_vtm], litl = op[B4NO_litl], wn = op[B4NO_weffnf];
  const double a = np[B4NP_noia], b = np[B4NP_noib], c = np[B4NP_noic], cq = coxe / q;
  const double x = (ab / (2.0 * vtm + vg)) * vde, N0 = vg * cq, Nl = N0 - N0 * x, dN = x * N0, Ns = (op[B4NO_cit] + op[B4NO_cdep0] + coxe) * (vtm / q);
  double dl = std::log(((op[B4NO_vds] - vde) / litl + np[B4NP_em]) / op[B4NO_esat]) * litl;
  if (!(dl > 0.0)) dl = 0.0;
  const double br = (0.5 * c) * ((N0 + Nl) * dN) + b * dN + a * std::log1p(dN / (Ns + Nl));
  const double s_inv = ((kT * ueff) * (q * q) * ids * il2 / (1.0e10 * ab * coxe)) * br + ((kT * dl) * (ids * ids) * il2 / (1.0e10 * wn)) * ((c * Nl * Nl + b * Nl + a) / ((Ns + Nl) * (Ns + Nl)));
  const double s_wi = (kT * a) * (ids * ids) / ((1.0e10 * leff) * wn * (Ns * Ns));
  *flicker = (s_inv > 0.0 && s_wi > 0.0) ? 1.0 / (1.0 / s_inv + 1.0 / s_wi) : 0.0;
}

static double reldev(double got, LD want) { return want == 0.0L ? (got == 0.0 ? 0.0 : INFINITY) : (double)(fabsl((LD)got - want) / fabsl(want)); }

int main(int argc, char**) {
  int bad = 0; long n_rows = 0;
  // ---- parameter packing: defaults by type, NaN means default, refusals ----
  {
    double row[CH_B4N_NPAR];
    b4n_pack(nullptr, 1.0, row);
    if (row[CH_B4N_noia] != 6.25e41 || row[CH_B4N_noib] != 3.125e26 || row[CH_B4N_noic] != 8.75e9 || row[CH_B4N_em] != 4.1e7 || row[CH_B4N_ef] != 1.0 || row[CH_B4N_af] != 1.0 ||
        row[CH_B4N_kf] != 0.0 || row[CH_B4N_ntnoi] != 1.0 || row[CH_B4N_fnoimod] != 1.0 || row[CH_B4N_tnoimod] != 0.0) { std::printf("n defaults wrong\n"); ++bad; }
    b4n_pack(nullptr, -1.0, row);
    if (row[CH_B4N_noia] != 6.188e40 || row[CH_B4N_noib] != 1.5e25 || row[CH_B4N_noic] != 8.75e9) { std::printf("p defaults wrong\n"); ++bad; }
    std::vector<double> g(CH_B4N_NPAR, NAN);
    g[CH_B4N_kf] = 3e-25; g[CH_B4N_fnoimod] = 0.0; g[CH_B4N_ef] = 0.9;
    b4n_pack(g.data(), -1.0, row);
    if (row[CH_B4N_kf] != 3e-25 || row[CH_B4N_fnoimod] != 0.0 || row[CH_B4N_ef] != 0.9 || row[CH_B4N_noia] != 6.188e40 || row[CH_B4N_ntnoi] != 1.0) { std::printf("NaN-means-default wrong\n"); ++bad; }
    // table: class 0 on model 1 (p, its own row), class 1 on model 0 (n, no row given), class 2 on a model index without a row
    std::vector<std::vector<double>> given(2); given[1] = g;
    std::vector<double> table; std::string err;
    int rc = b4n_table({1, 0, 5}, {-1.0, 1.0, 1.0}, given, table, err);
    if (rc != CH_OK || table.size() != 3u * CH_B4N_NPAR || table[CH_B4N_kf] != 3e-25 || table[CH_B4N_NPAR + CH_B4N_noia] != 6.25e41 || table[2 * CH_B4N_NPAR + CH_B4N_fnoimod] != 1.0) { std::printf("table wrong (%d)\n", rc); ++bad; }
    rc = b4n_table({}, {}, given, table, err);
    if (rc != CH_OK || table.size() != (size_t)CH_B4N_NPAR) { std::printf("empty table wrong\n"); ++bad; }
    given[0].assign(CH_B4N_NPAR, NAN); given[0][CH_B4N_tnoimod] = 1.0;
    rc = b4n_table({1, 0}, {-1.0, 1.0}, given, table, err);
    if (rc != CH_ERR_UNSUPPORTED || err.find("model card 0") == std::string::npos || err.find("tnoimod = 1") == std::string::npos) { std::printf("tnoimod 1 not refused: %d '%s'\n", rc, err.c_str()); ++bad; }
    given[0][CH_B4N_tnoimod] = 0.0; given[0][CH_B4N_fnoimod] = 2.0;
    rc = b4n_table({0}, {1.0}, given, table, err);
    if (rc != CH_ERR_UNSUPPORTED || err.find("fnoimod = 2") == std::string::npos) { std::printf("fnoimod 2 not refused\n"); ++bad; }
  }
  // ---- the records over a grid of operand rows ----
  struct Case { double op[B4NO_COUNT], np[CH_B4N_NPAR], T; };
  std::vector<Case> grid;
  const double coxe = 3.45e-11 / 1.2e-8;
  for (int form = 0; form < 3; ++form)            // 0: fnoimod 0 with kf, 1: fnoimod 1, 2: fnoimod 0 with kf = 0
    for (double type : {1.0, -1.0})
      for (double ids : {0.0, 3.0e-9, -4.7e-5, 2.1e-3})
        for (double vgst : {1.0e-9, 3.0e-3, 0.4, 2.7})
          for (double xd : {0.0, 0.02, 0.5, 1.3})      // vdseff as a multiple of vgst / abulk; 0: N0 = Nl exactly
            for (double over : {0.0, 0.9})             // vds - vdseff; 0 with em below esat (the p rows of the unified model): dLclm's logarithm is negative and clipped to 0
              for (double rds : {0.0, 35.0}) {
                Case c{};
                b4n_pack(nullptr, type, c.np);
                c.np[CH_B4N_fnoimod] = form == 1 ? 1.0 : 0.0;
                if (form == 0) { c.np[CH_B4N_kf] = 2.5e-26; c.np[CH_B4N_af] = 1.3; c.np[CH_B4N_ef] = 0.95; }
                if (form == 1 && type < 0) { c.np[CH_B4N_ntnoi] = 1.7; c.np[CH_B4N_em] = 2.0e6; }
                const double abulk = 1.15, vtm = 0.02585 * (type > 0 ? 1.0 : 1.33);
                c.T = vtm / 8.617087e-5;
                c.op[B4NO_ids] = ids; c.op[B4NO_ueff] = type > 0 ? 0.031 : 0.0094; c.op[B4NO_vgsteff] = vgst; c.op[B4NO_abulk] = abulk;
                c.op[B4NO_vdseff] = std::fmin(xd, 0.8) * vgst / abulk; c.op[B4NO_vds] = c.op[B4NO_vdseff] + over; c.op[B4NO_rds] = rds;
                c.op[B4NO_esat] = 2.0 * 8.0e4 / c.op[B4NO_ueff]; c.op[B4NO_litl] = 6.2e-8; c.op[B4NO_leff] = type > 0 ? 5.2e-7 : 9.9e-6;
                c.op[B4NO_weffnf] = 3.8e-6; c.op[B4NO_coxe] = coxe; c.op[B4NO_cdep0] = 4.1e-4; c.op[B4NO_cit] = form == 1 ? 1.0e-4 : 0.0; c.op[B4NO_vtm] = vtm;
                c.op[B4NO_qinv] = -coxe * 3.8e-6 * c.op[B4NO_leff] * vgst * (1.0 - 0.4 * std::fmin(xd, 0.8));
                grid.push_back(c);
              }
  double alt_max = 0.0, code_max = 0.0;
  std::vector<double> dev;
  for (const Case& c : grid) {
    B4NoiseRec rec[2]; LD rt, rf; double at, af;
    const int n = b4_noise_records(c.op, c.np, c.T, rec);
    ref_records(c.op, c.np, c.T, &rt, &rf);
    alt_records(c.op, c.np, c.T, &at, &af);
    if (n != 2 || rec[0].a != 0 || rec[0].b != 2 || rec[1].a != 0 || rec[1].b != 2 || rec[0].ex != 0.0 || rec[1].ex != c.np[CH_B4N_ef]) { std::printf("record shape wrong\n"); ++bad; }
    if (!(rec[0].pwr >= 0.0) || !(rec[1].pwr >= 0.0) || !std::isfinite(rec[0].pwr) || !std::isfinite(rec[1].pwr)) { std::printf("record not finite / negative\n"); ++bad; }
    if (c.np[CH_B4N_kf] == 0.0 && (int)c.np[CH_B4N_fnoimod] == 0 && rec[1].pwr != 0.0) { std::printf("kf = 0 leaves %g\n", rec[1].pwr); ++bad; }
    if (c.op[B4NO_ids] == 0.0 && rec[1].pwr != 0.0) { std::printf("ids = 0 leaves %g\n", rec[1].pwr); ++bad; }
    alt_max = std::fmax(alt_max, std::fmax(reldev(at, rt), reldev(af, rf)));
    dev.push_back(std::fmax(reldev(rec[0].pwr, rt), reldev(rec[1].pwr, rf)));
    code_max = std::fmax(code_max, dev.back());
    // with an argument: every 5th case as text, for the numpy yardstick (tests/test_host_b4_noise.py): operands | parameters | T | records
    if (argc > 1 && n_rows % 5 == 0) {
      std::printf("row");
      for (int q = 0; q < B4NO_COUNT; ++q) std::printf(" %.17g", c.op[q]);
      for (int q = 0; q < CH_B4N_NPAR; ++q) std::printf(" %.17g", c.np[q]);
      std::printf(" %.17g %.17g %.17g\n", c.T, rec[0].pwr, rec[1].pwr);
    }
    ++n_rows;
  }
  const double tol = std::fmax(8.0 * alt_max, 1e-14);
  for (double d : dev) if (!(d <= tol)) ++bad;
  // the unified model really ran on part of the grid and is not degenerate there
  { Case c = grid[0]; for (const Case& g : grid) if ((int)g.np[CH_B4N_fnoimod] == 1 && g.op[B4NO_ids] == 2.1e-3 && g.op[B4NO_vgsteff] == 0.4) { c = g; break; }
    B4NoiseRec rec[2]; b4_noise_records(c.op, c.np, c.T, rec);
    if (!(rec[1].pwr > 0.0)) { std::printf("unified model gave %g\n", rec[1].pwr); ++bad; } }
  std::printf("b4 noise: %ld operand rows, association-order deviation %.3e, tolerance %.3e, code deviation %.3e, %d bad\n", n_rows, alt_max, tol, code_max, bad);
  return bad ? 1 : 0;
}
