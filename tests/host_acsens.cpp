// Host-only test of the HIP-free half of ch_ac_sens (cedarsim.jl_amd/csrc/ch_acsens_host.hpp): the layout arithmetic of
// acsens_solve_kernel (odd row stride, panel width, workspace and frequency chunk), the step of the state term and the expansion of
// a complex sensitivity row from unknown order to MNA order.  Expected values are worked out by hand in the comments.  Built with
// sanitizers by tests/test_host_acsens.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "ch_acsens_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)

// the dynamic-LDS budget of the 64-lane kernel: 160 KiB minus its static __shared__ (a few hundred bytes), rounded down to 256 B.
// 163328 B = 20416 doubles is what 432 B of static variables leave.
static void panel_and_chunks() {
  const size_t budget = 20416;
  const int sizes[] = {1, 2, 16, 95, 96, 97, 4096};
  for (int nc : sizes) {
    const int lda = acsens_lda(nc);
    CHECK((lda & 1) == 1 && lda >= nc && lda <= nc + 1);
    CHECK(acsens_factor_doubles(nc) == (size_t)2 * nc * lda);
    for (int n_par : {1, 3, 8, 40, 200}) {
      const int kp = acsens_panel_columns(nc, n_par, budget);
      if (nc <= 96) {
        CHECK(kp >= 1 && kp <= n_par && kp <= ACSENS_MAX_PANEL);
        CHECK(acsens_factor_doubles(nc) + (size_t)2 * nc * kp <= budget);                       // what the launch asks for fits
        if (kp < n_par && kp < ACSENS_MAX_PANEL) CHECK(acsens_factor_doubles(nc) + (size_t)2 * nc * (kp + 1) > budget);   // and is the most that does
      } else if (nc == 97) {
        CHECK(kp == std::min(n_par, 8));   // arithmetic only (the launch sends 97 unknowns to the workspace variant): 20416 - 2*97*97 = 1598, 194 per column
      } else {
        CHECK(kp == 0);                    // the factors alone exceed the budget
      }
    }
  }
  // by hand: nc = 96 -> factors 2*96*97 = 18624, 1792 left, 192 per column -> 9;  nc = 95 -> 2*95*95 = 18050, 2366 left, 190 per column -> 12
  CHECK(acsens_panel_columns(96, 200, budget) == 9 && acsens_panel_columns(95, 200, budget) == 12);
  CHECK(acsens_panel_columns(96, 5, budget) == 5 && acsens_panel_columns(16, 200, budget) == 32 && acsens_panel_columns(1, 1, budget) == 1);
  CHECK(acsens_panel_columns(96, 200, 18624 + 191) == 0 && acsens_panel_columns(96, 200, 18624 + 192) == 1);
  CHECK(acsens_panel_columns(0, 1, budget) == 0 && acsens_panel_columns(4, 0, budget) == 0);
  // workspace of the 256-thread variant: factors + panel + permutation (ints, two to a double)
  CHECK(acsens_work_doubles(97, 3) == (size_t)2 * 97 * 97 + 2 * 97 * 3 + 49);
  CHECK(acsens_work_doubles(302, 3) == (size_t)2 * 302 * 303 + 2 * 302 * 3 + 151);
  CHECK(acsens_work_doubles(4096, 32) == (size_t)2 * 4096 * 4097 + (size_t)2 * 4096 * 32 + 2048);
  // chunks under 2^27 doubles: the 302-unknown ladder with 2 samples takes 400 frequencies in two launches (184975 doubles per
  // system, 369950 per frequency -> 362 frequencies); one 4096-unknown system with 32 columns takes 3 frequencies; never below 1
  CHECK(dense_work_chunk(acsens_work_doubles(302, 3), 2, 400) == 362);
  CHECK(dense_work_chunk(acsens_work_doubles(97, 1), 1, 7) == 7);
  CHECK(dense_work_chunk(acsens_work_doubles(4096, 32), 1, 61) == 3);
  CHECK(dense_work_chunk(acsens_work_doubles(4096, 32), 8, 61) == 1);
  for (int nc : {97, 256, 257, 4096}) for (int ny : {1, 2, 7}) {
    const int ch = dense_work_chunk(acsens_work_doubles(nc, 8), ny, 1000);
    CHECK(ch >= 1 && ch <= 1000);
    CHECK(ch == 1 || (size_t)ch * ny * acsens_work_doubles(nc, 8) <= DENSE_WORK_CAP);
  }
}

// The frequency chunk of the AC / noise solves and of the AC sensitivities is one function now: over a grid it must return what the
// two formulas it replaced return, written out here as they stood in launch_ac and in acsens_freq_chunk.  The workspace of a launch
// stays under the cap whenever the systems of ONE frequency do (where they do not, the chunk is 1 and hipMalloc decides).
static void frequency_chunks_as_before() {
  const size_t cap = (size_t)1 << 27;   // doubles
  CHECK(DENSE_WORK_CAP == cap);
  for (int ds : {1, 96, 97, 257, 4096}) for (int ny : {1, 3, 1024}) for (int n_freq : {1, 61, 2001}) {
    {   // launch_ac
      const size_t per = (size_t)2 * ds * (ds + 1);
      const int old_chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_freq, cap / (per * (size_t)ny)));
      const int chunk = dense_work_chunk(ac_system_doubles(ds), ny, n_freq);
      CHECK(ac_system_doubles(ds) == per && chunk == old_chunk);
      CHECK(chunk >= 1 && chunk <= n_freq);
      if (per * ny <= cap) CHECK((size_t)chunk * ny * per <= cap);
    }
    for (int n_par : {1, 32, 33, 134}) {   // launch_acsens
      const int kp = std::min(n_par, ACSENS_MAX_PANEL);
      const size_t per = acsens_work_doubles(ds, kp), per_freq = per * (size_t)std::max(1, ny);
      const int old_chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, n_freq), cap / per_freq));
      const int chunk = dense_work_chunk(per, ny, n_freq);
      CHECK(chunk == old_chunk);
      CHECK(chunk >= 1 && chunk <= n_freq);
      if (per_freq <= cap) CHECK((size_t)chunk * ny * per <= cap);
    }
  }
}

// the analysis of host_sens_steps.cpp: 5 nodes, 3 branches (n_mna = 8), 4 unknowns
//   node 1: unknown 0   node 2: known   node 3: merged into node 1 (unknown 0)   node 4: unknown 2   node 5: known
//   branch 0: unknown 1   branch 1: eliminated   branch 2: unknown 3
static Analysis hand_built() {
  Analysis A;
  A.n_nodes = 5; A.n_branch = 3; A.n_mna = 8; A.n_unk = 4; A.n_alias = 1;
  A.node_unknown = {-1, 0, -1, 0, 2, -1};
  A.node_known = {0, -1, 1, -1, -1, 2};
  A.branch_unknown = {1, -1, 3};
  A.known.resize(3);
  return A;
}

static void state_step() {
  Analysis A = hand_built();
  const double dv = 1.0 / 131072.0;
  // node unknowns are 0 and 2; 1 and 3 are branch currents
  { const double s[4] = {0.0, 5.0, 0.0, -7.0}; CHECK(acsens_state_eps(A, s, dv) == 0.0); }              // branch rows only: skipped
  { const double s[4] = {0.0, 0.0, 0.0, 0.0}; CHECK(acsens_state_eps(A, s, dv) == 0.0); }
  { const double s[4] = {-4.0, 1e9, 2.0, 1e9}; CHECK(acsens_state_eps(A, s, dv) == dv / 4.0); }          // the largest NODE shift is dv
  { const double s[4] = {0.5, 0.0, -0.25, 0.0}; CHECK(acsens_state_eps(A, s, dv) == dv * 2.0); }
  { const double s[4] = {1e300, 0.0, 1.0, 0.0}; const double e = acsens_state_eps(A, s, dv); CHECK(e > 0.0 && e == dv / 1e300 && e * 1e300 <= dv * 1.0000001); }   // huge s_k
  { const double s[4] = {std::numeric_limits<double>::infinity(), 0.0, 1.0, 0.0}; CHECK(acsens_state_eps(A, s, dv) == 0.0); }
  { const double s[4] = {1.0, 0.0, std::nan(""), 0.0}; CHECK(acsens_state_eps(A, s, dv) == 0.0); }
  { const double s[4] = {1e-320, 0.0, 0.0, 0.0}; const double e = acsens_state_eps(A, s, dv); CHECK(e == 0.0 || std::isfinite(e)); }   // dv / denormal overflows: skipped
  // G and C depend on the state only through MOSFETs and compiled devices
  CHECK(!acsens_state_dependent(A));
  EDev e; e.kind = K_R; e.nt = 2; e.hdev = 0; e.src = -1; e.mos = -1; for (int k = 0; k < NTERM; ++k) e.term[k] = -1;
  A.edev.push_back(e); CHECK(!acsens_state_dependent(A));
  e.kind = K_MOS; A.edev.push_back(e); CHECK(acsens_state_dependent(A));
  A.edev.back().kind = K_VA; CHECK(acsens_state_dependent(A));
}

static void mna_expansion() {
  const Analysis A = hand_built();
  const double zu[8] = {10.0, -10.5, 11.0, -11.5, 12.0, -12.5, 13.0, -13.5};   // (re, im) of unknowns 0..3
  std::vector<double> out(16, -1.0);
  acsens_expand_mna(A, zu, out.data());
  CHECK(out[0] == 10.0 && out[1] == -10.5);                 // node 1: unknown 0
  CHECK(out[2] == 0.0 && out[3] == 0.0);                    // node 2: known, no small signal
  CHECK(out[4] == 10.0 && out[5] == -10.5);                 // node 3: its representative's row
  CHECK(out[6] == 12.0 && out[7] == -12.5);                 // node 4: unknown 2
  CHECK(out[8] == 0.0 && out[9] == 0.0);                    // node 5: known
  CHECK(out[10] == 11.0 && out[11] == -11.5);               // branch 0: unknown 1
  CHECK(std::isnan(out[12]) && std::isnan(out[13]));        // branch 1: eliminated
  CHECK(out[14] == 13.0 && out[15] == -13.5);               // branch 2: unknown 3
  acsens_expand_mna(A, nullptr, out.data());                // a sample that was not served
  CHECK(std::isnan(out[0]) && std::isnan(out[1]) && out[2] == 0.0 && out[3] == 0.0 && std::isnan(out[4]) && std::isnan(out[7]) && out[8] == 0.0);
  CHECK(std::isnan(out[10]) && std::isnan(out[12]) && std::isnan(out[15]));
}

int main() {
  panel_and_chunks();
  frequency_chunks_as_before();
  state_step();
  mna_expansion();
  std::printf("acsens host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
