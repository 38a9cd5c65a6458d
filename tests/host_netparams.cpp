// Host-only test of the HIP-free half of ch_net_params (cedarsim.jl_amd/csrc/ch_netparams_host.hpp): the four P x P conversions
// against long-double arithmetic for P = 1, 2, 3, 8 (dense and strided storage), the exactly singular Yp, the checks of the ports and
// of the slots and the layout arithmetic of netparams_solve_kernel.  Built with sanitizers by tests/test_host_netparams.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ch_netparams_host.hpp"
#include "ch_sens_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)

typedef std::complex<long double> cld;
typedef std::vector<cld> Mat;   // P x P, row-major

static Mat mul(const Mat& A, const Mat& B, int P) {
  Mat C(P * P, cld(0));
  for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) for (int m = 0; m < P; ++m) C[i * P + j] += A[i * P + m] * B[m * P + j];
  return C;
}
// Gauss-Jordan with full row pivoting in long double: the reference inverse
static Mat inverse(Mat A, int P) {
  Mat B(P * P, cld(0));
  for (int i = 0; i < P; ++i) B[i * P + i] = 1;
  for (int k = 0; k < P; ++k) {
    int bi = k;
    for (int i = k; i < P; ++i) if (std::abs(A[i * P + k]) > std::abs(A[bi * P + k])) bi = i;
    for (int j = 0; j < P; ++j) { std::swap(A[k * P + j], A[bi * P + j]); std::swap(B[k * P + j], B[bi * P + j]); }
    const cld piv = A[k * P + k];
    for (int j = 0; j < P; ++j) { A[k * P + j] /= piv; B[k * P + j] /= piv; }
    for (int i = 0; i < P; ++i) if (i != k) {
      const cld l = A[i * P + k];
      for (int j = 0; j < P; ++j) { A[i * P + j] -= l * A[k * P + j]; B[i * P + j] -= l * B[k * P + j]; }
    }
  }
  return B;
}
static long double max_abs(const Mat& A) { long double m = 0; for (const cld& v : A) m = std::max(m, std::abs(v)); return m; }

// a deterministic generator (no <random>: the same figures everywhere)
static unsigned long long lcg = 88172645463325252ULL;
static double uni() { lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(lcg >> 11) / 9007199254740992.0 - 0.5; }

// max |got - want| / max |want| of a strided double matrix against a long-double one
static long double err_of(NetCMat got, const Mat& want, int P) {
  long double e = 0;
  for (int q = 0; q < P * P; ++q) { const double* v = net_at(got, q); e = std::max(e, std::abs(cld(v[0], v[1]) - want[q])); }
  return e / max_abs(want);
}
static bool all_nan(NetCMat m, int P) { for (int q = 0; q < P * P; ++q) { const double* v = net_at(m, q); if (!std::isnan(v[0]) || !std::isnan(v[1])) return false; } return true; }
static bool none_nan(NetCMat m, int P) { for (int q = 0; q < P * P; ++q) { const double* v = net_at(m, q); if (std::isnan(v[0]) || std::isnan(v[1])) return false; } return true; }

// A diagonally dominant admittance matrix (a passive network with a shunt path at every port: conditioning a few units) and a random
// derivative.  The bound: the conversions are an LU solve and two products of P x P matrices, a few P eps times the conditioning;
// 1e-13 leaves two orders over the 8-port figure (printed).
static void conversions() {
  const double z0s[8] = {50.0, 75.0, 25.0, 100.0, 50.0, 60.0, 30.0, 120.0};
  for (int P : {1, 2, 3, 8}) for (long st : {1L, 7L}) for (int trial = 0; trial < 4; ++trial) {
    std::vector<double> Y(2 * P * P * st, -7.0), dY(2 * P * P * st, -7.0), W(2 * P * P * st), S(2 * P * P * st), Z(2 * P * P * st), dS(2 * P * P * st), dZ(2 * P * P * st);
    Mat Yl(P * P), dYl(P * P), y(P * P), dy(P * P), I(P * P, cld(0));
    double rz[8];
    for (int i = 0; i < P; ++i) { rz[i] = std::sqrt(z0s[i]); I[i * P + i] = 1; }
    for (int i = 0; i < P; ++i) for (int j = 0; j < P; ++j) {
      const double re = (i == j ? 0.05 + 0.02 * (uni() + 0.5) : 0.01 * uni()) , im = 0.02 * uni(), dre = uni(), dim = uni();
      const long at = (long)(i * P + j) * st * 2;
      Y[at] = re; Y[at + 1] = im; dY[at] = dre; dY[at + 1] = dim;
      Yl[i * P + j] = cld(re, im); dYl[i * P + j] = cld(dre, dim);
      const long double sc = (long double)rz[i] * (long double)rz[j];
      y[i * P + j] = sc * Yl[i * P + j]; dy[i * P + j] = sc * dYl[i * P + j];
    }
    Mat ImY(P * P), IpY(P * P);
    for (int q = 0; q < P * P; ++q) { ImY[q] = I[q] - y[q]; IpY[q] = I[q] + y[q]; }
    const Mat Sl = mul(ImY, inverse(IpY, P), P), Zl = inverse(Yl, P);
    Mat IpS(P * P);
    for (int q = 0; q < P * P; ++q) IpS[q] = I[q] + Sl[q];
    Mat dSl = mul(mul(IpS, dy, P), IpS, P), dZl = mul(mul(Zl, dYl, P), Zl, P);
    for (cld& v : dSl) v *= -0.5L;
    for (cld& v : dZl) v = -v;
    NetCMat cY{Y.data(), st}, cdY{dY.data(), st};
    NetMat mW{W.data(), st}, mS{S.data(), st}, mZ{Z.data(), st}, mdS{dS.data(), st}, mdZ{dZ.data(), st};
    CHECK(net_y_to_s(cY, rz, mW, mS, P));
    net_dy_to_ds(net_const(mS), cdY, rz, mW, mdS, P);
    CHECK(net_y_to_z(cY, mW, mZ, P));
    net_dy_to_dz(net_const(mZ), cdY, mW, mdZ, P);
    const long double eS = err_of(net_const(mS), Sl, P), eZ = err_of(net_const(mZ), Zl, P), edS = err_of(net_const(mdS), dSl, P), edZ = err_of(net_const(mdZ), dZl, P);
    if (trial == 0 && st == 1) std::printf("P = %d: S %.1Le, Z %.1Le, dS %.1Le, dZ %.1Le\n", P, eS, eZ, edS, edZ);
    CHECK(eS <= 1e-13L); CHECK(eZ <= 1e-13L); CHECK(edS <= 1e-13L); CHECK(edZ <= 1e-13L);
    if (st > 1) CHECK(Y[2] == -7.0 && dY[3] == -7.0);   // the gaps of a strided input are not read as data, nor written
  }
  // closed forms: a 50 ohm shunt on one 50 ohm port is S = (1 - 1) / (1 + 1) = 0, Z = 50; a series 50 ohm between two 50 ohm ports
  double Y1[2] = {0.02, 0.0}, W1[2], S1[2], Z1[2], rz1[1] = {std::sqrt(50.0)};
  CHECK(net_y_to_s(NetCMat{Y1, 1}, rz1, NetMat{W1, 1}, NetMat{S1, 1}, 1) && std::fabs(S1[0]) <= 2e-16 && S1[1] == 0.0);
  CHECK(net_y_to_z(NetCMat{Y1, 1}, NetMat{W1, 1}, NetMat{Z1, 1}, 1) && std::fabs(Z1[0] - 50.0) <= 1e-14 && Z1[1] == 0.0);
}

// the exactly singular Yp of a series-only two-port: S exists (1/3, 2/3), Z and dZ are NaN, nothing else is
static void singular() {
  const double g = 0.02;
  double Y[8] = {g, 0, -g, 0, -g, 0, g, 0}, dY[8] = {1, 0, -1, 0, -1, 0, 1, 0}, W[8], S[8], Z[8], dS[8], dZ[8], rz[2] = {std::sqrt(50.0), std::sqrt(50.0)};
  CHECK(net_y_to_s(NetCMat{Y, 1}, rz, NetMat{W, 1}, NetMat{S, 1}, 2));
  CHECK(std::fabs(S[0] - 1.0 / 3.0) <= 4e-16 && std::fabs(S[2] - 2.0 / 3.0) <= 4e-16 && std::fabs(S[4] - 2.0 / 3.0) <= 4e-16 && std::fabs(S[6] - 1.0 / 3.0) <= 4e-16);
  net_dy_to_ds(NetCMat{S, 1}, NetCMat{dY, 1}, rz, NetMat{W, 1}, NetMat{dS, 1}, 2);
  CHECK(none_nan(NetCMat{S, 1}, 2) && none_nan(NetCMat{dS, 1}, 2));
  // d S11 / d g of S11 = 1 / (1 + 2 g z0): -2 z0 / (1 + 2 g z0)^2 = -100 / 9
  CHECK(std::fabs(dS[0] + 100.0 / 9.0) <= 1e-13);
  CHECK(!net_y_to_z(NetCMat{Y, 1}, NetMat{W, 1}, NetMat{Z, 1}, 2));
  CHECK(all_nan(NetCMat{Z, 1}, 2));
  net_fill_nan(NetMat{dZ, 1}, 2);   // (what the kernel does after a breakdown)
  CHECK(all_nan(NetCMat{dZ, 1}, 2) && none_nan(NetCMat{Y, 1}, 2));
  double Yn[2] = {CH_NAN, 0.0}, Wn[2], Sn[2], r1[1] = {1.0};   // a failed solve stays NaN
  CHECK(!net_y_to_s(NetCMat{Yn, 1}, r1, NetMat{Wn, 1}, NetMat{Sn, 1}, 1) && std::isnan(Sn[0]));
  double Y0[2] = {0.0, 0.0}, Z0[2];   // an open port: Z does not exist
  CHECK(!net_y_to_z(NetCMat{Y0, 1}, NetMat{Wn, 1}, NetMat{Z0, 1}, 1) && std::isnan(Z0[0]));
}

static HDev device(int kind, int a, int b, int src = -1, int branch = -1) {
  HDev d; std::memset(&d, 0, sizeof(d));
  d.kind = kind; d.node[0] = a; d.node[1] = b; d.ipar[0] = src; d.mult = 1.0; d.branch = branch; d.eliminated = false;
  return d;
}
static HSource source(double ac) {
  HSource s; s.kind = CH_SRC_DC; s.dc = 0.0; s.ac = ac; std::memset(s.par, 0, sizeof(s.par));
  return s;
}
static bool says(const char* w, const char* text) { return w && std::string(w).find(text) != std::string::npos; }

// nodes 1, 2, 3; devices 0: r 1-2, 1: vp1 1 -> 0 (branch 0, source 0), 2: vp2 2 -> 0 (branch 1, source 1), 3: vdd 3 -> 0 (branch 2,
// source 2, eliminated), 4: i 0 -> 1 (source 3)
static void port_checks() {
  std::vector<HDev> dev = {device(CH_DEV_R, 1, 2), device(CH_DEV_V, 1, 0, 0, 0), device(CH_DEV_V, 2, 0, 1, 1), device(CH_DEV_V, 3, 0, 2, 2), device(CH_DEV_I, 0, 1, 3)};
  dev[3].eliminated = true;
  std::vector<HSource> src = {source(1.0), source(1.0), source(0.0), source(0.0)};
  Analysis A;
  A.n_nodes = 3; A.n_branch = 3; A.n_mna = 6; A.n_unk = 4;
  A.node_unknown = {-1, 0, 1, -1};
  A.branch_unknown = {2, 3, -1};
  std::vector<int> u; int bad = -1;
  const int both[2] = {1, 2}, swapped[2] = {2, 1}, twice[2] = {1, 1}, with_r[2] = {1, 0}, with_vdd[2] = {1, 3}, none[1] = {7};
  CHECK(netparams_port_check(dev, src, A, 2, both, u, bad) == nullptr && bad == 0 && u.size() == 2 && u[0] == 2 && u[1] == 3);
  CHECK(netparams_port_check(dev, src, A, 2, swapped, u, bad) == nullptr && u[0] == 3 && u[1] == 2);   // the order given is the port order
  CHECK(says(netparams_port_check(dev, src, A, 2, twice, u, bad), "twice") && bad == 2);
  CHECK(says(netparams_port_check(dev, src, A, 2, with_r, u, bad), "not a voltage source") && bad == 2);
  CHECK(says(netparams_port_check(dev, src, A, 2, with_vdd, u, bad), "eliminated") && bad == 2);
  CHECK(says(netparams_port_check(dev, src, A, 1, none, u, bad), "no such device") && bad == 1);
  CHECK(says(netparams_port_check(dev, src, A, 0, both, u, bad), "between 1 and 8") && bad == 0);
  CHECK(says(netparams_port_check(dev, src, A, 9, both, u, bad), "between 1 and 8") && bad == 0);
  CHECK(says(netparams_port_check(dev, src, A, 1, both, u, bad), "no port carries") && bad == 0);     // vp2 is driven but is no port
  { std::vector<HSource> s2 = src; s2[1].ac = 0.5; CHECK(says(netparams_port_check(dev, s2, A, 2, both, u, bad), "|ac| = 1") && bad == 2); }
  { std::vector<HSource> s2 = src; s2[3].ac = 1e-3; CHECK(says(netparams_port_check(dev, s2, A, 2, both, u, bad), "no port carries") && bad == 0); }
  { std::vector<HDev> d2 = dev; d2[1].mult = 2.0; CHECK(says(netparams_port_check(d2, src, A, 2, both, u, bad), "multiplier") && bad == 1); }
  { Analysis B = A; B.branch_unknown[1] = -1; CHECK(says(netparams_port_check(dev, src, B, 2, both, u, bad), "eliminated") && bad == 2); }
  const int same[3] = {4, 4, 4}, split[3] = {4, 4, 5};
  CHECK(netparams_split_port(same, 3) == -1 && netparams_split_port(split, 3) == 2 && netparams_split_port(split, 2) == -1 && netparams_split_port(split, 1) == -1);
  // slots: 0 vp1's multiplier, 1 the resistor's multiplier, 2 vp2's DC value, 3 the resistor's value, 4 vp2's multiplier
  const std::vector<int> kind = {CH_SLOT_DEV_MULT, CH_SLOT_DEV_MULT, CH_SLOT_SRC_DC, CH_SLOT_DEV_PAR, CH_SLOT_DEV_MULT}, a = {1, 0, 1, 0, 2};
  CHECK(netparams_slot_moves_b(kind, a, 0, 2, both) && netparams_slot_moves_b(kind, a, 4, 2, both));
  CHECK(!netparams_slot_moves_b(kind, a, 1, 2, both) && !netparams_slot_moves_b(kind, a, 2, 2, both) && !netparams_slot_moves_b(kind, a, 3, 2, both));
  CHECK(!netparams_slot_moves_b(kind, a, 4, 1, both));   // with vp1 the only port, vp2's multiplier is an ordinary slot
}

// the dynamic-LDS budget of the 64-lane kernel: 160 KiB minus its static __shared__ (the 96-entry permutation), rounded down to 256 B:
// 163328 B = 20416 doubles
static void layout() {
  const size_t budget = 20416;
  CHECK(CH_NET_MAX_PORTS == 8);
  for (int P = 1; P <= 8; ++P) {
    for (int nc = 1; nc <= 97; ++nc) {
      const size_t lda = (size_t)(nc | 1);
      CHECK(netparams_lds_doubles(nc, P) == 2 * nc * lda + (size_t)2 * nc * P);
      CHECK(netparams_work_doubles(nc, P) == netparams_lds_doubles(nc, P) + ((size_t)nc + 1) / 2);
      if (nc <= 96) CHECK(netparams_lds_doubles(nc, P) <= budget);
    }
    CHECK(netparams_work_doubles(4096, P) == (size_t)2 * 4096 * 4097 + (size_t)2 * 4096 * P + 2048);
  }
  CHECK(netparams_lds_doubles(96, 8) == 18624 + 1536 && netparams_lds_doubles(96, 8) * sizeof(double) == 161280);
  CHECK(netparams_lds_doubles(96, 8) * sizeof(double) <= 160 * 1024);        // the cap of 8 ports: (96, 8) fits 160 KB ...
  CHECK(netparams_lds_doubles(96, 10) * sizeof(double) > 160 * 1024);        // ... (96, 10) does not: 164352 B
  CHECK(netparams_lds_doubles(96, 2) == 18624 + 384);                        // two ports: loopgain_solve_kernel's figure
  CHECK(netparams_work_doubles(97, 8) == (size_t)2 * 97 * 97 + 1552 + 49);
  // what launch_freq_chunks makes of it: under 2^27 doubles per launch, never below one frequency
  CHECK(dense_work_chunk(netparams_work_doubles(97, 8), 1, 7) == 7);
  const size_t per = netparams_work_doubles(4096, 8);                        // 2*4096*4097 + 65536 + 2048 = 33630208
  CHECK(per == 33630208);
  CHECK(dense_work_chunk(per, 1, 61) == 3 && dense_work_chunk(per, 4, 61) == 1);
}

int main() {
  conversions();
  singular();
  port_checks();
  layout();
  std::printf("netparams host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
