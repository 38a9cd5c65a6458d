// Host-only test of the HIP-free half of ch_dc_sens (cedarsim.jl_amd/csrc/ch_sens_host.hpp): the finite-difference step rule for
// every slot kind, the step plan of a call (SensPlan) on a hand-built slot table and the expansion of a sensitivity column from
// unknown order to MNA order.  Expected values are worked out by
// hand in the comments; steps are powers of two so every comparison is exact.  Built with sanitizers by tests/test_host_sens_steps.py.
#include <cmath>
#include <cstdio>
#include <vector>
#include "ch_sens_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)

static bool fwd(SensStep s, double h) { return !s.central && s.h == h; }
static bool cen(SensStep s, double h) { return s.central && s.h == h; }

static void step_rule() {
  const double r = 1.0 / 131072.0;   // 2^-17
  CHECK(SENS_REL_STEP == r && SENS_GMIN_STEP == 1.0 / 1048576.0);
  // residual linear in p: forward difference, absolute step 1 whatever p is — p = 0 and negative p included
  for (double p : {0.0, 5.0, -3.3, 1e-15, 1e12}) {
    CHECK(fwd(sens_step(CH_SLOT_SRC_DC, 0, false, false, p, r, 0.0), 1.0));
    CHECK(fwd(sens_step(CH_SLOT_SRC_PAR, 0, false, false, p, r, 0.0), 1.0));
    CHECK(fwd(sens_step(CH_SLOT_DEV_MULT, 0, false, false, p, r, 0.0), 1.0));
    CHECK(fwd(sens_step(CH_SLOT_DEV_PAR, CH_DEV_VCVS, false, false, p, r, 0.0), 1.0));
    CHECK(fwd(sens_step(CH_SLOT_DEV_PAR, CH_DEV_VCCS, true, false, p, r, 0.0), 1.0));
  }
  // a source that sets a known node under a MOSFET / compiled device reaches the residual through that device: central, relative
  CHECK(cen(sens_step(CH_SLOT_SRC_DC, 0, false, true, 4.0, r, 0.0), 4.0 / 131072.0));
  CHECK(cen(sens_step(CH_SLOT_SRC_DC, 0, false, true, 0.0, r, 0.0), r));
  CHECK(cen(sens_step(CH_SLOT_SRC_PAR, 0, true, true, -2.0, r, 0.0), 2.0 / 131072.0));
  CHECK(fwd(sens_step(CH_SLOT_DEV_MULT, 0, false, true, 3.0, r, 0.0), 1.0));   // (the flag concerns source slots only)
  // gmin: 2^-20 S absolute while every device uses it linearly ...
  CHECK(fwd(sens_step(CH_SLOT_GMIN, 0, false, false, 1e-12, r, 0.0), 1.0 / 1048576.0));
  CHECK(fwd(sens_step(CH_SLOT_GMIN, 0, false, false, 0.0, r, 0.0), 1.0 / 1048576.0));
  // ... central and relative as soon as a compiled Verilog-A instance is present: 2^-17 * 2^-40
  CHECK(cen(sens_step(CH_SLOT_GMIN, 0, true, false, std::ldexp(1.0, -40), r, 0.0), std::ldexp(1.0, -57)));
  CHECK(cen(sens_step(CH_SLOT_GMIN, 0, true, false, 0.0, r, 0.0), r));
  // everything else: central, h = rel_step * |p|; p = 0 -> h = rel_step; negative p -> positive step
  const int nonlinear_dev[] = {CH_DEV_R, CH_DEV_C, CH_DEV_L, CH_DEV_MOS};
  for (int dk : nonlinear_dev) {
    CHECK(cen(sens_step(CH_SLOT_DEV_PAR, dk, false, false, 1024.0, r, 0.0), 1024.0 / 131072.0));
    CHECK(cen(sens_step(CH_SLOT_DEV_PAR, dk, false, false, -1024.0, r, 0.0), 1024.0 / 131072.0));
    CHECK(cen(sens_step(CH_SLOT_DEV_PAR, dk, false, false, 0.0, r, 0.0), r));
  }
  CHECK(cen(sens_step(CH_SLOT_MODEL_PAR, 0, false, false, -0.5, r, 0.0), 0.5 / 131072.0));
  CHECK(cen(sens_step(CH_SLOT_MODEL_PAR, 0, false, false, 0.0, r, 0.0), r));
  CHECK(cen(sens_step(CH_SLOT_TEMP, 0, false, false, 32.0, r, 0.0), 32.0 / 131072.0));
  CHECK(cen(sens_step(CH_SLOT_TEMP, 0, false, false, -64.0, r, 0.0), 64.0 / 131072.0));
  CHECK(cen(sens_step(CH_SLOT_VA_PAR, 0, true, false, 2.0, r, 0.0), 2.0 / 131072.0));
  CHECK(cen(sens_step(CH_SLOT_VA_PAR, 0, true, false, 0.0, r, 0.0), r));
  // another rel_step; a non-positive one falls back to the default
  CHECK(cen(sens_step(CH_SLOT_DEV_PAR, CH_DEV_R, false, false, 8.0, 0.25, 0.0), 2.0));
  CHECK(cen(sens_step(CH_SLOT_DEV_PAR, CH_DEV_R, false, false, 8.0, 0.0, 0.0), 8.0 / 131072.0));
  // abs_step > 0 replaces the step and keeps the kind of difference; <= 0 leaves the rule alone
  CHECK(cen(sens_step(CH_SLOT_DEV_PAR, CH_DEV_R, false, false, 8.0, r, 0.125), 0.125));
  CHECK(fwd(sens_step(CH_SLOT_GMIN, 0, false, false, 1e-12, r, std::ldexp(1.0, -30)), std::ldexp(1.0, -30)));
  CHECK(cen(sens_step(CH_SLOT_GMIN, 0, true, false, 1e-12, r, std::ldexp(1.0, -30)), std::ldexp(1.0, -30)));
  CHECK(fwd(sens_step(CH_SLOT_SRC_DC, 0, false, false, 2.0, r, -1.0), 1.0));
}

// Hand-built analysis, 5 nodes and 3 branches (n_mna = 8):
//   node 1: unknown 0          node 2: known 1 = +2*src0 - 3*src1 + 0.5*src0   node 3: merged into node 1 by a 0 V ammeter (unknown 0)
//   node 4: unknown 2          node 5: known 2 = -1*src1
//   branch 0: unknown 1        branch 1: eliminated                            branch 2: unknown 3
static Analysis hand_built() {
  Analysis A;
  A.n_nodes = 5; A.n_branch = 3; A.n_mna = 8; A.n_unk = 4; A.n_alias = 1;
  A.node_unknown = {-1, 0, -1, 0, 2, -1};
  A.node_known = {0, -1, 1, -1, -1, 2};
  A.branch_unknown = {1, -1, 3};
  A.known.resize(3);
  A.known[1].terms = {{0, 2.0}, {1, -3.0}, {0, 0.5}};
  A.known[2].terms = {{1, -1.0}};
  // devices: a resistor on known node 1, a MOSFET with its source on known node 2 (fed by source 1), a compiled device on unknowns only
  { EDev e; e.kind = K_R; e.nt = 4; e.hdev = 0; e.src = -1; e.mos = -1; for (int k = 0; k < NTERM; ++k) e.term[k] = -1; e.term[0] = -2; e.term[1] = 0; A.edev.push_back(e);
    e.kind = K_MOS; e.term[0] = 0; e.term[1] = 2; e.term[2] = -3; e.term[3] = -1; A.edev.push_back(e);
    e.kind = K_VA; e.nt = 2; e.term[0] = 0; e.term[1] = 2; e.term[2] = -2; A.edev.push_back(e); }   // term[2] is beyond nt: not a terminal
  return A;
}

static void mna_expansion() {
  const Analysis A = hand_built();
  CHECK(sens_known_deriv(A.known[1], 0, 1.0) == 2.5 && sens_known_deriv(A.known[1], 1, 1.0) == -3.0 && sens_known_deriv(A.known[1], 2, 1.0) == 0.0);
  CHECK(sens_known_deriv(A.known[0], 0, 1.0) == 0.0 && sens_known_deriv(A.known[2], 1, 4.0) == -4.0);
  const std::vector<char> nl = sens_sources_feeding_nonlinear(A, 3);
  CHECK(nl.size() == 3 && nl[0] == 0 && nl[1] == 1 && nl[2] == 0);
  const double su[4] = {10.0, 11.0, 12.0, 13.0};
  std::vector<double> out(8, -1.0);
  // a slot that is no source: known nodes 0
  sens_expand_mna(A, su, -1, 0.0, out.data());
  CHECK(out[0] == 10.0 && out[1] == 0.0 && out[2] == 10.0 && out[3] == 12.0 && out[4] == 0.0);
  CHECK(out[5] == 11.0 && std::isnan(out[6]) && out[7] == 13.0);
  // the slot of source 0, unit derivative: node 2 gets 2 + 0.5, node 5 (fed by source 1 only) 0
  sens_expand_mna(A, su, 0, 1.0, out.data());
  CHECK(out[1] == 2.5 && out[4] == 0.0 && out[0] == 10.0 && out[2] == 10.0 && std::isnan(out[6]));
  // the slot of source 1 with d(source value)/dp = 0.5
  sens_expand_mna(A, su, 1, 0.5, out.data());
  CHECK(out[1] == -1.5 && out[4] == -0.5);
  // a failed operating point: unknown rows NaN, known rows still exact
  sens_expand_mna(A, nullptr, 0, 1.0, out.data());
  CHECK(std::isnan(out[0]) && out[1] == 2.5 && std::isnan(out[2]) && std::isnan(out[3]) && out[4] == 0.0 && std::isnan(out[5]) && std::isnan(out[6]) && std::isnan(out[7]));
}

// The step plan of one call on the analysis above (source 1 feeds the MOSFET, source 0 no nonlinear device).  Slot table:
//   slot 0: parameter of device 0, a resistor      slot 1: DC value of source 0      slot 2: parameter of source 1      slot 3: gmin
//   slot 4: multiplier of device 0
// Six parameters — slots 0, 1, 2, 3, 4 and slot 0 again with abs_step = 2^-3 — over three samples, rel_step = 2^-17:
//   k  slot  values p            difference                       h                          den
//   0  0     1024, 0, -512       central (a resistance)           2^-7, 2^-17, 2^-8          2^-6, 2^-16, 2^-7
//   1  1     2, 0, -3            forward (linear branch row)      1, 1, 1                    1, 1, 1
//   2  2     4, 0, -2            central (reaches the MOSFET)     2^-15, 2^-17, 2^-16        2^-14, 2^-16, 2^-15
//   3  3     2^-40, 0, 2^-30     forward, 2^-20 S (no Verilog-A)  2^-20 each                 2^-20 each
//            the same            central (a Verilog-A instance)   2^-57, 2^-17, 2^-47        2^-56, 2^-16, 2^-46
//   4  4     2, 0, -1            forward                          1, 1, 1                    1, 1, 1
//   5  0     1024, 0, -512       central, abs_step                2^-3 each                  2^-2 each
// Every p +- h below is exact in double precision (at most 47 significant bits).
static void step_plan() {
  Analysis A = hand_built();
  const std::vector<int> slot_kind = {CH_SLOT_DEV_PAR, CH_SLOT_SRC_DC, CH_SLOT_SRC_PAR, CH_SLOT_GMIN, CH_SLOT_DEV_MULT}, slot_a = {0, 0, 1, 0, 0};
  std::vector<HDev> dev(1);
  dev[0].kind = CH_DEV_R;
  const double val[5][3] = {{1024.0, 0.0, -512.0}, {2.0, 0.0, -3.0}, {4.0, 0.0, -2.0}, {std::ldexp(1.0, -40), 0.0, std::ldexp(1.0, -30)}, {2.0, 0.0, -1.0}};
  const int32_t ids[6] = {0, 1, 2, 3, 4, 0};
  const double abs_step[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.125};
  const ch_sens_opts opt = {1.0 / 131072.0, abs_step};
  auto value = [&](int id, int s) { return val[id][s]; };
  const int S = 3;
  auto L = [](int e) { return std::ldexp(1.0, e); };
  for (int with_va = 0; with_va <= 1; ++with_va) {
    A.wide = with_va != 0;
    const SensPlan P = sens_plan(slot_kind, slot_a, dev, A, 3, 6, ids, S, value, opt);
    CHECK(P.n_par == 6 && P.S == 3 && P.slot == std::vector<int>({0, 1, 2, 3, 4, 0}));
    CHECK(P.kind == std::vector<int>({CH_SLOT_DEV_PAR, CH_SLOT_SRC_DC, CH_SLOT_SRC_PAR, CH_SLOT_GMIN, CH_SLOT_DEV_MULT, CH_SLOT_DEV_PAR}));
    CHECK(P.central == std::vector<int>({1, 0, 1, with_va, 0, 1}));
    CHECK(P.src_of == std::vector<int>({-1, 0, 1, -1, -1, -1}));
    CHECK(!P.is_src(0) && P.is_src(1) && P.is_src(2) && !P.is_src(3) && !P.is_src(4) && !P.is_src(5));
    const double h[6][3] = {{L(-7), L(-17), L(-8)}, {1.0, 1.0, 1.0}, {L(-15), L(-17), L(-16)},
                            {with_va ? L(-57) : L(-20), with_va ? L(-17) : L(-20), with_va ? L(-47) : L(-20)}, {1.0, 1.0, 1.0}, {0.125, 0.125, 0.125}};
    for (int k = 0; k < 6; ++k) {
      const std::vector<double> plus = P.values(k, +1), minus = P.values(k, -1);
      CHECK((int)plus.size() == S && (int)minus.size() == S);
      for (int s = 0; s < S; ++s) {
        const double p = val[ids[k]][s];
        CHECK(P.p[k * S + s] == p && P.h[k * S + s] == h[k][s]);
        CHECK(P.den[k * S + s] == (P.central[k] ? 2.0 : 1.0) * h[k][s]);
        CHECK(plus[s] == p + h[k][s] && minus[s] == p - h[k][s] && plus[s] != p && minus[s] != p);
      }
    }
    // spelled out for one entry of each row: the values the evaluations are made at
    CHECK(P.values(0, +1)[0] == 1024.0078125 && P.values(0, -1)[2] == -512.00390625 && P.values(0, -1)[1] == -L(-17));
    CHECK(P.values(1, +1)[2] == -2.0 && P.values(1, +1)[1] == 1.0 && P.den[1 * S + 0] == 1.0);
    CHECK(P.values(2, -1)[0] == 4.0 - L(-15) && P.den[2 * S + 2] == L(-15));
    CHECK(P.values(3, +1)[1] == (with_va ? L(-17) : L(-20)) && P.den[3 * S + 0] == (with_va ? L(-56) : L(-20)));
    CHECK(P.values(4, +1)[2] == 0.0 && P.values(5, +1)[0] == 1024.125 && P.values(5, -1)[1] == -0.125 && P.den[5 * S + 1] == 0.25);
  }
}

// LDS layout of the solve kernel: 2*96*97 doubles hold an nc x lda matrix, lda odd
static void lds_layout() {
  const size_t budget = (size_t)2 * 96 * 97;
  for (int nc = 1; nc <= 96; ++nc) {
    const int kc = sens_lds_columns(nc, budget);
    CHECK(kc >= 1);
    CHECK((sens_lda(nc, kc) & 1) == 1 && sens_lda(nc, kc) >= nc + kc);
    CHECK((size_t)nc * sens_lda(nc, kc) <= budget);
    CHECK((sens_lda(nc, 1) & 1) == 1 && sens_lda(nc, 1) >= nc + 1);
  }
  CHECK(sens_lds_columns(96, budget) == 97 && sens_lds_columns(80, budget) == 151);   // 18624/96 - 97, 18624/80 - 81
}

// Columns and blocks per launch of the solve kernel: over a grid the functions must return what launch_sens computed inline before
// they moved here, written out as it stood.  The workspace of a launch stays under the cap whenever one block does.
static void launch_chunks_as_before() {
  const size_t cap = (size_t)1 << 27;   // doubles
  CHECK(DENSE_WORK_CAP == cap);
  for (int ds : {1, 96, 97, 257, 4096}) for (int nblk : {1, 3, 1024}) for (int n_par : {1, 32, 33, 134}) {
    const int old_kmax = std::min(n_par, 32);
    const size_t old_per = (size_t)ds * sens_lda(ds, old_kmax);
    const int old_bchunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nblk, cap / old_per));
    const int kmax = sens_work_columns(n_par), bchunk = sens_block_chunk(ds, kmax, nblk);
    CHECK(kmax == old_kmax && sens_work_doubles(ds, kmax) == old_per && bchunk == old_bchunk);
    CHECK(bchunk >= 1 && bchunk <= nblk);
    if (old_per <= cap) CHECK((size_t)bchunk * old_per <= cap);
    // the general rule with several systems per item, against the same formula
    for (int n : {1, 61, 2001}) {
      const int ch = dense_work_chunk(old_per, nblk, n);
      CHECK(ch == (int)std::max<size_t>(1, std::min<size_t>((size_t)n, cap / (old_per * (size_t)nblk))));
      CHECK(ch >= 1 && (old_per * nblk > cap || (size_t)ch * nblk * old_per <= cap));
    }
    if (ds <= 96) CHECK(sens_lds_chunk_columns(ds) == std::max(1, sens_lds_columns(ds, (size_t)2 * 96 * 97)));
  }
}

int main() {
  step_rule();
  mna_expansion();
  step_plan();
  lds_layout();
  launch_chunks_as_before();
  std::printf("sens host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
