// ch_netparams_host.hpp — HIP-free half of the N-port network analysis, ch_net_params: the checks of the ports and of the slots, the
// P x P conversions Yp -> S, Yp -> Z, dYp -> dS, dYp -> dZ and the layout arithmetic of netparams_solve_kernel.  DESIGN.md 2.7k has
// the definition in words.
//
// Ports are voltage sources `vpJ a b`, numbered in the order given.  Run k puts 1 V AC on port k and 0 V on the others (ideal sources:
// AC shorts); a source's branch current flows from + through the source to -, so the current entering the network at port j is -i_pj:
//   Yp[j][k] = -x_k[row_i(j)],   y = sqrt(z0) Yp sqrt(z0),   S = (I - y)(I + y)^-1 = (I + y)^-1 (I - y),   Z = Yp^-1,
//   dS = -1/2 (I + S)(sqrt(z0) dYp sqrt(z0))(I + S),   dZ = -Z dYp Z.
// The conversions run on the host and, unchanged, in netparams_convert_kernel (one thread per (frequency, sample)): a matrix is
// a pointer and an element stride, so the same code walks a dense host array and the rows of the device layout.
// Tested as a stand-alone program (tests/host_netparams.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

#include "ch_measure_host.hpp"   // CH_MEAS_HD, CH_MEAS_NOCONTRACT
#include "ch_analysis.hpp"
#include "ch_sens_host.hpp"      // clu_*: the layout of the in-place complex LU

namespace chip {

constexpr int CH_NET_MAX_PORTS = 8;   // 96 unknowns and a panel of 8 columns still fit the LDS (netparams_lds_doubles)
enum { CH_NET_S = 0, CH_NET_Y = 1, CH_NET_Z = 2 };   // measure rows: kind * P^2 + j * P + k

// ---- the ports ----
// null, or why the devices `port_devs` cannot be the ports; `bad` then holds the offending port's number (1-based; 0: the list
// itself).  u_ip: the global unknown of every port's branch current.
inline const char* netparams_port_check(const std::vector<HDev>& dev, const std::vector<HSource>& src, const Analysis& A, int n_ports, const int* port_devs,
                                        std::vector<int>& u_ip, int& bad) {
  u_ip.clear(); bad = 0;
  if (n_ports < 1 || n_ports > CH_NET_MAX_PORTS || !port_devs) return "between 1 and 8 ports";
  std::vector<char> is_port(src.size(), 0);
  for (int j = 0; j < n_ports; ++j) {
    bad = j + 1;
    const int pd = port_devs[j];
    if (pd < 0 || pd >= (int)dev.size()) return "no such device";
    for (int q = 0; q < j; ++q) if (port_devs[q] == pd) return "appears twice";
    const HDev& d = dev[pd];
    if (d.kind != CH_DEV_V) return "is not a voltage source";
    if (d.branch < 0 || d.branch >= A.n_branch || d.eliminated || A.branch_unknown[d.branch] < 0)
      return "its branch current was eliminated (a port must reach the engine as an AC-driven source: |ac| = 1)";
    const int si = d.ipar[0];
    if (si < 0 || si >= (int)src.size() || src[si].ac != 1.0) return "its source must carry |ac| = 1";
    if (d.mult != 1.0) return "its multiplier must be 1";
    is_port[si] = 1;
    u_ip.push_back(A.branch_unknown[d.branch]);
  }
  bad = 0;
  for (int k = 0; k < (int)src.size(); ++k) if (!is_port[k] && src[k].ac != 0.0) return "a source that is no port carries an AC magnitude (every other AC excitation must be off)";
  return nullptr;
}

// the first port (0-based) whose branch current lies in another block than port 1's, or -1.  comp[j]: the block of port j
inline int netparams_split_port(const int* comp, int n_ports) {
  for (int j = 1; j < n_ports; ++j) if (comp[j] != comp[0]) return j;
  return -1;
}

// true when slot `id` would move a right-hand side: a port's own multiplier (it scales the branch current the ports read)
inline bool netparams_slot_moves_b(const std::vector<int>& slot_kind, const std::vector<int>& slot_a, int id, int n_ports, const int* port_devs) {
  if (slot_kind[id] != CH_SLOT_DEV_MULT) return false;
  for (int j = 0; j < n_ports; ++j) if (slot_a[id] == port_devs[j]) return true;
  return false;
}

// ---- P x P complex matrices: element (i, j) at p[((i * P + j) * st) * 2], real and imaginary part side by side ----
struct NetMat { double* p; long st; };
struct NetCMat { const double* p; long st; };
CH_MEAS_HD NetCMat net_const(NetMat m) { NetCMat c; c.p = m.p; c.st = m.st; return c; }
CH_MEAS_HD double* net_at(NetMat m, int e) { return m.p + (long)e * m.st * 2; }
CH_MEAS_HD const double* net_at(NetCMat m, int e) { return m.p + (long)e * m.st * 2; }
CH_MEAS_HD void net_fill_nan(NetMat m, int P) { for (int e = 0; e < P * P; ++e) { double* v = net_at(m, e); v[0] = CH_NAN; v[1] = CH_NAN; } }

// A X = B in place (X over B, A destroyed): Gaussian elimination with the family's pivot rule (largest |re| + |im|, lowest row on
// ties; a pivot that is zero, NaN or beyond 1e300 is a breakdown: false, B holds nothing)
CH_MEAS_HD bool net_lu_solve(NetMat A, NetMat B, int P) { CH_MEAS_NOCONTRACT
  for (int k = 0; k < P; ++k) {
    double best = -1.0; int bi = k;
    for (int i = k; i < P; ++i) { const double* v = net_at(A, i * P + k); const double m = std::fabs(v[0]) + std::fabs(v[1]); if (m > best) { best = m; bi = i; } }
    if (!(best > 0.0 && best < 1e300)) return false;
    if (bi != k) for (int j = 0; j < P; ++j) {
      double* a0 = net_at(A, k * P + j); double* a1 = net_at(A, bi * P + j);
      double t = a0[0]; a0[0] = a1[0]; a1[0] = t; t = a0[1]; a0[1] = a1[1]; a1[1] = t;
      double* b0 = net_at(B, k * P + j); double* b1 = net_at(B, bi * P + j);
      t = b0[0]; b0[0] = b1[0]; b1[0] = t; t = b0[1]; b0[1] = b1[1]; b1[1] = t;
    }
    const double* pv = net_at(A, k * P + k);
    const double pr = pv[0], pi = pv[1], den = 1.0 / (pr * pr + pi * pi), ir = pr * den, ii = -pi * den;   // 1/pivot
    for (int i = k + 1; i < P; ++i) {
      const double* l = net_at(A, i * P + k);
      const double lr = l[0] * ir - l[1] * ii, li = l[0] * ii + l[1] * ir;
      if (lr == 0.0 && li == 0.0) continue;
      for (int j = k + 1; j < P; ++j) {
        const double* u = net_at(A, k * P + j); double* a = net_at(A, i * P + j);
        a[0] -= lr * u[0] - li * u[1]; a[1] -= lr * u[1] + li * u[0];
      }
      for (int j = 0; j < P; ++j) {
        const double* u = net_at(B, k * P + j); double* b = net_at(B, i * P + j);
        b[0] -= lr * u[0] - li * u[1]; b[1] -= lr * u[1] + li * u[0];
      }
    }
  }
  for (int k = P - 1; k >= 0; --k) {
    const double* pv = net_at(A, k * P + k);
    const double pr = pv[0], pi = pv[1], den = 1.0 / (pr * pr + pi * pi);
    for (int j = 0; j < P; ++j) {
      double* b = net_at(B, k * P + j);
      const double br = b[0], bi_ = b[1];
      b[0] = (br * pr + bi_ * pi) * den; b[1] = (bi_ * pr - br * pi) * den;
      for (int i = 0; i < k; ++i) {
        const double* u = net_at(A, i * P + k); double* x = net_at(B, i * P + j);
        x[0] -= u[0] * b[0] - u[1] * b[1]; x[1] -= u[0] * b[1] + u[1] * b[0];
      }
    }
  }
  return true;
}

// S = (I + y)^-1 (I - y), y = rz Yp rz with rz[j] = sqrt(z0[j]).  W: P x P of work space.  False (S is NaN): I + y broke down
CH_MEAS_HD bool net_y_to_s(NetCMat Y, const double* rz, NetMat W, NetMat S, int P) { CH_MEAS_NOCONTRACT
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) {
    const double* y = net_at(Y, i * P + j); const double sc = rz[i] * rz[j], yr = sc * y[0], yi = sc * y[1], d = i == j ? 1.0 : 0.0;
    double* w = net_at(W, i * P + j); double* s = net_at(S, i * P + j);
    w[0] = d + yr; w[1] = yi; s[0] = d - yr; s[1] = -yi;
  }
  if (net_lu_solve(W, S, P)) return true;
  net_fill_nan(S, P);
  return false;
}

// Z = Yp^-1.  False (Z is NaN): Yp broke down, which a series-only network legitimately does
CH_MEAS_HD bool net_y_to_z(NetCMat Y, NetMat W, NetMat Z, int P) {
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) {
    const double* y = net_at(Y, i * P + j); double* w = net_at(W, i * P + j); double* z = net_at(Z, i * P + j);
    w[0] = y[0]; w[1] = y[1]; z[0] = i == j ? 1.0 : 0.0; z[1] = 0.0;
  }
  if (net_lu_solve(W, Z, P)) return true;
  net_fill_nan(Z, P);
  return false;
}

// out = scale * (L + shift I)(ra D rb)(L + shift I), D scaled by ra[i] * rb[j] (null: 1).  W takes the left product
CH_MEAS_HD void net_congruence(NetCMat L, double shift, NetCMat D, const double* r, double scale, NetMat W, NetMat out, int P) { CH_MEAS_NOCONTRACT
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) {
    double sr = 0.0, si = 0.0;
    for (int m = 0; m < P; ++m) {
      const double* l = net_at(L, i * P + m); const double* d = net_at(D, m * P + j);
      const double lr = l[0] + (i == m ? shift : 0.0), li = l[1], sc = r ? r[m] * r[j] : 1.0, dr = sc * d[0], di = sc * d[1];
      sr += lr * dr - li * di; si += lr * di + li * dr;
    }
    double* w = net_at(W, i * P + j); w[0] = sr; w[1] = si;
  }
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) {
    double sr = 0.0, si = 0.0;
    for (int m = 0; m < P; ++m) {
      const double* w = net_at(W, i * P + m); const double* l = net_at(L, m * P + j);
      const double lr = l[0] + (m == j ? shift : 0.0), li = l[1];
      sr += w[0] * lr - w[1] * li; si += w[0] * li + w[1] * lr;
    }
    double* o = net_at(out, i * P + j); o[0] = scale * sr; o[1] = scale * si;
  }
}
// dS = -1/2 (I + S)(rz dYp rz)(I + S)
CH_MEAS_HD void net_dy_to_ds(NetCMat S, NetCMat dY, const double* rz, NetMat W, NetMat dS, int P) { net_congruence(S, 1.0, dY, rz, -0.5, W, dS, P); }
// dZ = -Z dYp Z
CH_MEAS_HD void net_dy_to_dz(NetCMat Z, NetCMat dY, NetMat W, NetMat dZ, int P) { net_congruence(Z, 0.0, dY, nullptr, -1.0, W, dZ, P); }

// ---- layout of netparams_solve_kernel: the complex factors and a panel of P right-hand sides; the 256-thread variant adds the row
// permutation (through launch_freq_chunks, as loopgain_solve_kernel) ----
inline size_t netparams_lds_doubles(int nc, int P) { return clu_factor_doubles(nc) + clu_panel_doubles(nc, P); }
inline size_t netparams_work_doubles(int nc, int P) { return netparams_lds_doubles(nc, P) + clu_perm_doubles(nc); }

}  // namespace chip
