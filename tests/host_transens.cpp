// Host-only test of the HIP-free half of ch_tran_sens (cedarsim.jl_amd/csrc/ch_transens_host.hpp): the ring, row and dump layout, the
// column-chunk rule at the shape edges of transens_step_kernel (1, 16, 96 unknowns in LDS; 97 on the 256-thread path), the test
// that refuses a slot which moves a break point, the derivative of a known node's value at a time, and the scalar one-step recursion
// against a 2 x 2 case worked out by hand in the comments.  Built with sanitizers by tests/test_host_transens.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "ch_transens_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)
static bool near(double a, double b, double tol) { return std::fabs(a - b) <= tol; }

static void layout_and_chunks() {
  // rings [NSLOT][n_par][S][n_unk]
  CHECK(NSLOT == 8);
  CHECK(transens_ring_doubles(3, 2, 5) == 240);
  CHECK(transens_ring_index(0, 0, 0, 0, 3, 2, 5) == 0);
  CHECK(transens_ring_index(0, 0, 1, 0, 3, 2, 5) == 5);
  CHECK(transens_ring_index(0, 1, 0, 0, 3, 2, 5) == 10);
  CHECK(transens_ring_index(1, 0, 0, 0, 3, 2, 5) == 30);
  CHECK(transens_ring_index(7, 2, 1, 4, 3, 2, 5) == 239);
  CHECK(transens_row_doubles(4, 3, 2) == 24);
  CHECK(transens_dump_index(0, 0, 0, 6, 11) == 0 && transens_dump_index(2, 5, 10, 6, 11) == 3 * 66 - 1);
  // columns beside an nc x nc matrix in 2*96*97 = 18624 doubles of LDS, odd row stride: 18624/nc - nc - 1
  const size_t budget = (size_t)2 * 96 * 97;
  CHECK(transens_chunk_columns(1) == 18622 && transens_chunk_columns(16) == 1147 && transens_chunk_columns(96) == 97);
  CHECK(transens_chunk_columns(97) == 32 && transens_chunk_columns(4096) == 32);   // 256-thread path: 32 columns per launch
  for (int nc : {1, 16, 96}) {
    const int kc = transens_chunk_columns(nc);
    CHECK(sens_lda(nc, kc) % 2 == 1);
    CHECK(transens_lds_doubles(nc, kc) <= budget);
    CHECK(transens_lds_doubles(nc, kc + 2) > budget);   // (kc + 1 may share the odd stride of kc)
  }
  CHECK(transens_lds_doubles(96, 97) == (size_t)96 * 193);
  CHECK(transens_n_chunks(96, 97) == 1 && transens_n_chunks(96, 98) == 2 && transens_n_chunks(96, 100) == 2 && transens_n_chunks(96, 1) == 1);
  CHECK(transens_n_chunks(97, 32) == 1 && transens_n_chunks(97, 33) == 2 && transens_n_chunks(97, 100) == 4);
  CHECK(transens_n_chunks(1, 18622) == 1 && transens_n_chunks(16, 1148) == 2);
}

static HSource pulse(double v1, double v2, double td, double tr, double tf, double pw, double per) {
  HSource s; s.kind = CH_SRC_PULSE; s.dc = v1;
  const double p[7] = {v1, v2, td, tr, tf, pw, per};
  for (int k = 0; k < CH_SRC_NPAR; ++k) s.par[k] = k < 7 ? p[k] : 0.0;
  return s;
}
static HSource sine(double vo, double va, double f) {
  HSource s; s.kind = CH_SRC_SIN; s.dc = vo;
  const double p[7] = {vo, va, f, 0.0, 0.0, 0.0, std::numeric_limits<double>::infinity()};
  for (int k = 0; k < CH_SRC_NPAR; ++k) s.par[k] = k < 7 ? p[k] : 0.0;
  return s;
}
static std::vector<double> pars_of(const std::vector<HSource>& v) {
  std::vector<double> p;
  for (const HSource& s : v) p.insert(p.end(), s.par, s.par + CH_SRC_NPAR);
  return p;
}

static void break_points() {
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<HSource> srcs = {pulse(0.0, 1.0, 1e-9, 1e-9, 1e-9, 5e-9, inf), sine(0.5, 0.25, 1e6)};
  const std::vector<double> own = pars_of(srcs);
  auto moved = [&](int src, int field, double dv) { std::vector<double> p = own; p[(size_t)src * CH_SRC_NPAR + field] += dv; return transens_moves_breakpoints(srcs, own, p, 1, 0.0, 2e-8); };
  CHECK(!moved(0, 0, 1e-3) && !moved(0, 1, 1e-3) && !moved(0, 1, -1e-3));   // PULSE levels: the times stay
  CHECK(moved(0, 2, 1e-12) && moved(0, 3, 1e-12) && moved(0, 4, 1e-12) && moved(0, 5, 1e-12));   // td, tr, tf, pw
  CHECK(!moved(0, 6, 1.0));                                                 // an infinite period stays infinite
  CHECK(!moved(1, 0, 1e-3) && !moved(1, 1, 1e-3) && !moved(1, 2, 10.0) && !moved(1, 5, 1.0));   // SIN offset, amplitude, frequency, phase
  CHECK(moved(1, 3, 0.5e-9));                                               // a SIN's delay is a break point (not at a corner of the PULSE)
  CHECK(!transens_moves_breakpoints(srcs, own, own, 1, 0.0, 2e-8));
  // outside the span nothing moves
  CHECK(!transens_moves_breakpoints(srcs, own, [&] { std::vector<double> p = own; p[2] += 1e-12; return p; }(), 1, 1e-7, 2e-7));
  // two parameter sets: a move in the second set alone counts
  std::vector<double> own2 = own; own2.insert(own2.end(), own.begin(), own.end());
  std::vector<double> p2 = own2; p2[own.size() + 2] += 1e-12;
  CHECK(transens_moves_breakpoints(srcs, own2, p2, 2, 0.0, 2e-8));
}

static void known_nodes() {
  std::vector<HSource> srcs = {pulse(0.0, 1.0, 1e-9, 1e-9, 1e-9, 5e-9, std::numeric_limits<double>::infinity()), sine(0.5, 0.25, 1e6)};
  KnownDef k; k.terms = {{0, 1.0}, {1, -2.0}};
  double pp[CH_SRC_NPAR], p0[CH_SRC_NPAR];
  // amplitude of the SIN, forward step 1: value = vo + va sin(2 pi f t); at t = T/4 the derivative is 1, times the coefficient -2
  for (int j = 0; j < CH_SRC_NPAR; ++j) { p0[j] = srcs[1].par[j]; pp[j] = p0[j]; }
  pp[1] += 1.0;
  CHECK(near(transens_known_deriv(k, srcs, 1, false, pp, 0.5, p0, 0.5, 1.0, 0.25e-6, 1), -2.0, 1e-12));
  CHECK(near(transens_known_deriv(k, srcs, 1, false, pp, 0.5, p0, 0.5, 1.0, 0.75e-6, 1), +2.0, 1e-12));   // 3T/4: sin = -1
  CHECK(near(transens_known_deriv(k, srcs, 1, false, pp, 0.5, p0, 0.5, 1.0, 0.5e-6, 1), 0.0, 1e-12));     // T/2
  // offset of the SIN: 1 at any time
  for (int j = 0; j < CH_SRC_NPAR; ++j) pp[j] = p0[j];
  pp[0] += 1.0;
  CHECK(near(transens_known_deriv(k, srcs, 1, false, pp, 0.5, p0, 0.5, 1.0, 0.3e-6, 1), -2.0, 1e-12));
  // upper level of the PULSE with step 0.5: 0 before the edge, half way up the edge 0.5, on the plateau 1 (coefficient +1)
  for (int j = 0; j < CH_SRC_NPAR; ++j) { p0[j] = srcs[0].par[j]; pp[j] = p0[j]; }
  pp[1] += 0.5;
  CHECK(transens_known_deriv(k, srcs, 0, false, pp, 0.0, p0, 0.0, 0.5, 0.5e-9, 1) == 0.0);
  CHECK(near(transens_known_deriv(k, srcs, 0, false, pp, 0.0, p0, 0.0, 0.5, 1.5e-9, 1), 0.5, 1e-12));
  CHECK(near(transens_known_deriv(k, srcs, 0, false, pp, 0.0, p0, 0.0, 0.5, 4e-9, 1), 1.0, 1e-12));
  // the slot IS the value: the coefficient, exactly; a slot that is no source slot: 0; a source the node does not depend on: 0
  CHECK(transens_known_deriv(k, srcs, 1, true, p0, 0.5, p0, 0.5, 1.0, 0.1e-6, 1) == -2.0);
  CHECK(transens_known_deriv(k, srcs, -1, false, p0, 0.5, p0, 0.5, 1.0, 0.1e-6, 1) == 0.0);
  KnownDef other; other.terms = {{0, 1.0}};
  CHECK(transens_known_deriv(other, srcs, 1, true, p0, 0.5, p0, 0.5, 1.0, 0.1e-6, 1) == 0.0);
}

static void scalar_step() {
  // G = [2 1; 1 3], C = [1 0; 0 2], alpha = (1, -1), one history point w_1 = (1, 2), df = (1, 0), dq = (0, 1):
  //   A = G + C = [3 1; 1 5], b = -(df + dq - w_1) = -((1,0) + (0,1) - (1,2)) = (0, 1), det A = 14
  //   s = (1/14) (5*0 - 1*1, -1*0 + 3*1) = (-1/14, 3/14);   w = C s + dq = (-1/14, 6/14 + 1) = (-1/14, 10/7)
  const double G[4] = {2, 1, 1, 3}, C[4] = {1, 0, 0, 2}, df[2] = {1, 0}, dq[2] = {0, 1}, alpha[2] = {1, -1}, w1[2] = {1, 2};
  const double* hist[1] = {w1};
  double s[2], w[2];
  CHECK(transens_step_scalar(2, G, C, df, dq, alpha, 1, hist, s, w));
  CHECK(near(s[0], -1.0 / 14.0, 1e-15) && near(s[1], 3.0 / 14.0, 1e-15));
  CHECK(near(w[0], -1.0 / 14.0, 1e-15) && near(w[1], 10.0 / 7.0, 1e-15));
  // order 0 (a DC solve): alpha0 = 0, no history: G s = -df -> det G = 5, s = -(1/5)(3*1, -1*1) = (-3/5, 1/5); w = C s + dq = (-3/5, 2/5 + 1)
  const double a0[1] = {0.0};
  CHECK(transens_step_scalar(2, G, C, df, dq, a0, 0, nullptr, s, w));
  CHECK(near(s[0], -0.6, 1e-15) && near(s[1], 0.2, 1e-15) && near(w[0], -0.6, 1e-15) && near(w[1], 1.4, 1e-15));
  // a zero pivot in front: rows are exchanged.  G = [0 1; 1 0], df = (1, 2): s = (-2, -1)
  const double P[4] = {0, 1, 1, 0}, Z[4] = {0, 0, 0, 0}, df2[2] = {1, 2}, z2[2] = {0, 0};
  CHECK(transens_step_scalar(2, P, Z, df2, z2, a0, 0, nullptr, s, w));
  CHECK(s[0] == -2.0 && s[1] == -1.0 && w[0] == 0.0 && w[1] == 0.0);
  // two history points: b = -(df + a0 dq + a1 w1 + a2 w2) with alpha = (1.5, -2, 0.5), w1 = (1, 2), w2 = (2, 2), C = I, G = I:
  //   A = 2.5 I, b = -((1,0) + 1.5 (0,1) - (2,4) + (1,1)) = -(0, -1.5) = (0, 1.5): s = (0, 0.6), w = s + dq = (0, 1.6)
  const double I2[4] = {1, 0, 0, 1}, al3[3] = {1.5, -2.0, 0.5}, w2[2] = {2, 2};
  const double* hist2[2] = {w1, w2};
  CHECK(transens_step_scalar(2, I2, I2, df, dq, al3, 2, hist2, s, w));
  CHECK(near(s[0], 0.0, 1e-15) && near(s[1], 0.6, 1e-15) && near(w[0], 0.0, 1e-15) && near(w[1], 1.6, 1e-15));
  // a matrix that does not factor
  CHECK(!transens_step_scalar(2, Z, Z, df, dq, a0, 0, nullptr, s, w));
  const double R1[4] = {1, 2, 2, 4};
  CHECK(!transens_step_scalar(2, R1, Z, df, dq, a0, 0, nullptr, s, w));
}

int main() {
  layout_and_chunks();
  break_points();
  known_nodes();
  scalar_step();
  std::printf("transens host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
