// Host-only test of the HIP-free half of ch_loop_gain (cedarsim.jl_amd/csrc/ch_loopgain_host.hpp): the combination u -> T and
// du -> dT against long-double arithmetic, the checks of the probe and of the slots, the sign of the current-injection right-hand
// side and the layout arithmetic of loopgain_solve_kernel.  Expected values are worked out by hand in the comments.  Built with
// sanitizers by tests/test_host_loopgain.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ch_loopgain_host.hpp"
#include "ch_sens_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)

typedef std::complex<long double> cld;
static bool close_to(double re, double im, cld want, long double rel) {
  return std::abs(cld(re, im) - want) <= rel * std::max((long double)1e-300, std::abs(want));
}

// T = u / (1 - u) and dT = du / (1 - u)^2 against long double, over magnitudes and phases of u; the bound is a few roundings of the
// double formula (4 eps) times the conditioning |1 - u|^-1 is NOT included: u is kept away from 1 here, the pole is checked apart
static void combination() {
  const double mags[] = {1e-12, 1e-3, 0.3, 0.9, 2.0, 37.0, 1e6, 1e12};
  for (double m : mags) for (int k = 0; k < 16; ++k) {
    const double ph = 0.39269908169872414 * k + 0.1, ur = m * std::cos(ph), ui = m * std::sin(ph);
    const cld u((long double)ur, (long double)ui), one(1.0L, 0.0L);
    double tr, ti;
    loopgain_T_of_u(ur, ui, tr, ti);
    CHECK(close_to(tr, ti, u / (one - u), 8e-16L));
    const double dur = 0.7 * m + 1e-3, dui = -1.3 * m;
    double dr, di;
    loopgain_dT_of_du(ur, ui, dur, dui, dr, di);
    CHECK(close_to(dr, di, cld((long double)dur, (long double)dui) / ((one - u) * (one - u)), 1.6e-15L));
  }
  double tr, ti;
  loopgain_T_of_u(2.0 / 3.0, 0.0, tr, ti);            // the test loop at DC: T = 2
  CHECK(std::fabs(tr - 2.0) <= 4e-16 * 2.0 * 3.0 && ti == 0.0);
  loopgain_T_of_u(-2.0 / 3.0, 0.0, tr, ti);           // its reversed probe: T = -0.4
  CHECK(std::fabs(tr + 0.4) <= 4e-16 && ti == 0.0);
  loopgain_T_of_u(0.0, 0.0, tr, ti);
  CHECK(tr == 0.0 && ti == 0.0);
  loopgain_T_of_u(1.0, 0.0, tr, ti);                  // 1 - u = 0 is no failure: what IEEE gives, nothing traps
  CHECK(!std::isfinite(tr) || !std::isfinite(ti));
  double dr, di;
  loopgain_dT_of_du(1.0, 0.0, 1.0, 0.0, dr, di);
  CHECK(!std::isfinite(dr) || !std::isfinite(di));
  loopgain_dT_of_du(0.0, 0.0, 3.0, -4.0, dr, di);     // u = 0: dT = du
  CHECK(dr == 3.0 && di == -4.0);
  loopgain_T_of_u(CH_NAN, 0.0, tr, ti);               // a failed solve stays NaN
  CHECK(std::isnan(tr));
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

// nodes 1 (x), 2 (y), 3 (held by vdd); devices 0: r 1-0, 1: vprobe 1 -> 2 (branch 0, source 0), 2: vdd 3 -> 0 (branch 1, source 1,
// eliminated: node 3 is known), 3: vback 2 -> 1 (branch 2, source 2), 4: v3 3 -> 2 (branch 3), 5: i 0 -> 1 (source 3)
static void probe_checks() {
  std::vector<HDev> dev = {device(CH_DEV_R, 1, 0), device(CH_DEV_V, 1, 2, 0, 0), device(CH_DEV_V, 3, 0, 1, 1), device(CH_DEV_V, 2, 1, 2, 2),
                           device(CH_DEV_V, 3, 2, 2, 3), device(CH_DEV_I, 0, 1, 3)};
  dev[2].eliminated = true;
  std::vector<HSource> src = {source(1.0), source(0.0), source(1.0), source(0.0)};
  Analysis A;
  A.n_nodes = 3; A.n_branch = 4; A.n_mna = 7; A.n_unk = 5;
  A.node_unknown = {-1, 0, 1, -1};          // ground, x, y, the held node
  A.branch_unknown = {2, -1, 3, 4};
  LoopGainProbe P;
  src[2].ac = 0.0;
  CHECK(loopgain_probe_check(dev, src, A, 1, P) == nullptr && P.u_x == 0 && P.u_ip == 2);
  const char* w = loopgain_probe_check(dev, src, A, 0, P);
  CHECK(w && std::string(w).find("not a voltage source") != std::string::npos && P.u_x == -1);
  w = loopgain_probe_check(dev, src, A, 5, P);
  CHECK(w && std::string(w).find("not a voltage source") != std::string::npos);
  CHECK(loopgain_probe_check(dev, src, A, -1, P) != nullptr && loopgain_probe_check(dev, src, A, 6, P) != nullptr);
  w = loopgain_probe_check(dev, src, A, 2, P);                                         // + node held by ideal sources
  CHECK(w && std::string(w).find("+ node") != std::string::npos);
  w = loopgain_probe_check(dev, src, A, 4, P);
  CHECK(w && std::string(w).find("+ node") != std::string::npos);
  { std::vector<HDev> d2 = dev; d2[1].node[0] = 0; w = loopgain_probe_check(d2, src, A, 1, P); CHECK(w && std::string(w).find("+ node") != std::string::npos); }   // ground
  { Analysis B = A; B.branch_unknown[0] = -1; w = loopgain_probe_check(dev, src, B, 1, P); CHECK(w && std::string(w).find("eliminated") != std::string::npos); }
  { std::vector<HDev> d2 = dev; d2[1].eliminated = true; w = loopgain_probe_check(d2, src, A, 1, P); CHECK(w && std::string(w).find("eliminated") != std::string::npos); }
  { std::vector<HSource> s2 = src; s2[0].ac = 0.5; w = loopgain_probe_check(dev, s2, A, 1, P); CHECK(w && std::string(w).find("|ac| = 1") != std::string::npos); }
  { std::vector<HSource> s2 = src; s2[3].ac = 1e-3; w = loopgain_probe_check(dev, s2, A, 1, P); CHECK(w && std::string(w).find("another source") != std::string::npos); }
  // the reversed probe (device 3, y -> x) is as good a probe: its + node is y
  { std::vector<HSource> s2 = src; s2[0].ac = 0.0; s2[2].ac = 1.0; CHECK(loopgain_probe_check(dev, s2, A, 3, P) == nullptr && P.u_x == 1 && P.u_ip == 3); }
  // slots: 0 the probe's multiplier, 1 the resistor's multiplier, 2 the probe's DC value, 3 the resistor's value
  const std::vector<int> kind = {CH_SLOT_DEV_MULT, CH_SLOT_DEV_MULT, CH_SLOT_SRC_DC, CH_SLOT_DEV_PAR}, a = {1, 0, 0, 0};
  CHECK(loopgain_slot_moves_b(kind, a, 0, 1) && !loopgain_slot_moves_b(kind, a, 1, 1) && !loopgain_slot_moves_b(kind, a, 2, 1) && !loopgain_slot_moves_b(kind, a, 3, 1));
  CHECK(!loopgain_slot_moves_b(kind, a, 0, 3));   // another probe: device 1's multiplier is an ordinary slot
}

// `I 0 x ac=1`: the engine's current-source stamp is F[first terminal] += i, F[second] -= i (current leaving a node counts positive)
// and b = -dF/d(ac), so the node the current is driven INTO, the second terminal, takes +1.  (That the engine's b has this sign is
// what the GPU test against two ac() runs pins; here only that the rule the driver calls says so.)
static void bi_sign() {
  CHECK(LOOPGAIN_BI_TERMINAL == 1 && loopgain_bi_entry(LOOPGAIN_BI_TERMINAL) == 1.0 && loopgain_bi_entry(0) == -1.0);
}

// the dynamic-LDS budget of the 64-lane kernel: 160 KiB minus its static __shared__ (the 96-entry permutation), rounded down to 256 B:
// 163328 B = 20416 doubles
static void layout() {
  const size_t budget = 20416;
  for (int nc : {1, 2, 4, 63, 64, 95, 96, 97, 4096}) {
    const int lda = loopgain_lda(nc);
    CHECK((lda & 1) == 1 && lda >= nc && lda <= nc + 1);
    CHECK(loopgain_lds_doubles(nc) == (size_t)2 * nc * lda + (size_t)4 * nc);
    CHECK(loopgain_work_doubles(nc) == loopgain_lds_doubles(nc) + ((size_t)nc + 1) / 2);
    if (nc <= 96) CHECK(loopgain_lds_doubles(nc) <= budget);
  }
  CHECK(loopgain_lds_doubles(96) == 18624 + 384 && loopgain_lds_doubles(4) == 40 + 16);
  CHECK(loopgain_lds_doubles(97) == (size_t)2 * 97 * 97 + 388);            // 19206: arithmetic only, 97 unknowns go to the workspace variant
  CHECK(loopgain_work_doubles(97) == 19206 + 49);
  // what launch_freq_chunks makes of it: under 2^27 doubles per launch, never below one frequency
  CHECK(dense_work_chunk(loopgain_work_doubles(97), 1, 7) == 7);
  const size_t per = loopgain_work_doubles(4096);                          // 2*4096*4097 + 16384 + 2048 = 33581056
  CHECK(per == 33581056);
  CHECK(dense_work_chunk(per, 1, 61) == 3 && dense_work_chunk(per, 4, 61) == 1);
}

int main() {
  combination();
  probe_checks();
  bi_sign();
  layout();
  std::printf("loopgain host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
