// Host-only test of the HIP-free half of ch_noise_sens (cedarsim.jl_amd/csrc/ch_noisesens_host.hpp): the layout arithmetic of
// noisesens_solve_kernel (odd row stride, resident part, panel width, LDS and workspace sizes), the frequency chunk under the cap and
// the MOSFET noise-parameter table with the extra row of a perturbed instance column.  Expected values are worked out by hand in the
// comments.  Built with sanitizers by tests/test_host_noisesens.py.
#include <cmath>
#include <cstdio>
#include <vector>
#include "ch_noisesens_host.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)

// the dynamic-LDS budget of the 64-lane kernel: 160 KiB minus its static __shared__ (384 B, the 96-entry permutation: the compiler
// drops the reduction arrays of the one-wavefront variant), rounded down to 256 B: 163328 B = 20416 doubles
static void panels_and_workspace() {
  const size_t budget = 20416;
  const int sizes[] = {1, 2, 16, 95, 96, 97, 4096};
  for (int nc : sizes) {
    const int lda = noisesens_lda(nc);
    CHECK((lda & 1) == 1 && lda >= nc && lda <= nc + 1);
    CHECK(noisesens_resident_doubles(nc) == (size_t)2 * nc * lda + (size_t)2 * nc);
    for (int n_par : {0, 1, 3, 8, 17, 40, 200}) {
      const int kp = noisesens_panel_columns(nc, n_par, budget);
      if (nc <= 96) {
        CHECK(kp >= (n_par ? 1 : 0) && kp <= n_par && kp <= NOISESENS_MAX_PANEL);
        CHECK(noisesens_lds_doubles(nc, kp) <= budget);                                                            // what the launch asks for fits
        if (kp < n_par && kp < NOISESENS_MAX_PANEL) CHECK(noisesens_lds_doubles(nc, kp + 1) > budget);             // and is the most that does
      } else if (nc == 97) {
        CHECK(kp == std::min(n_par, 7));   // arithmetic only (97 unknowns go to the workspace variant): 20416 - 2*97*97 - 194 = 1404, 194 per column
      } else {
        CHECK(kp == -1);                   // the factors alone exceed the budget
      }
      CHECK(noisesens_work_doubles(nc, noisesens_work_columns(n_par)) == noisesens_resident_doubles(nc) + (size_t)2 * nc * std::min(n_par, 32) + ((size_t)nc + 1) / 2);
    }
  }
  // by hand: nc = 96 -> 2*96*97 + 192 = 18816 resident, 1600 left, 192 per column -> 8;  nc = 95 -> 2*95*95 + 190 = 18240, 2176 left, 190 per column -> 11
  CHECK(noisesens_panel_columns(96, 200, budget) == 8 && noisesens_panel_columns(95, 200, budget) == 11);
  CHECK(noisesens_panel_columns(96, 5, budget) == 5 && noisesens_panel_columns(16, 200, budget) == 32 && noisesens_panel_columns(1, 1, budget) == 1);
  CHECK(noisesens_panel_columns(96, 200, 18816 + 191) == -1 && noisesens_panel_columns(96, 200, 18816 + 192) == 1);
  CHECK(noisesens_panel_columns(96, 0, 18816) == 0 && noisesens_panel_columns(96, 0, 18815) == -1);               // the y-only launch needs the resident part alone
  CHECK(noisesens_panel_columns(0, 1, budget) == -1 && noisesens_panel_columns(4, -1, budget) == -1);
  CHECK(noisesens_lds_doubles(96, 8) == 18816 + 1536 && noisesens_lds_doubles(1, 0) == 4);
  CHECK(noisesens_work_columns(0) == 0 && noisesens_work_columns(5) == 5 && noisesens_work_columns(33) == 32);
  CHECK(noisesens_work_doubles(97, 3) == (size_t)2 * 97 * 97 + 194 + 2 * 97 * 3 + 49);
  CHECK(noisesens_work_doubles(302, 0) == (size_t)2 * 302 * 303 + 604 + 151);
  CHECK(noisesens_work_doubles(4096, 32) == (size_t)2 * 4096 * 4097 + 8192 + (size_t)2 * 4096 * 32 + 2048);
}

// chunks under DENSE_WORK_CAP = 2^27 doubles
static void chunk_rule() {
  // the 302-unknown ladder, 2 samples, 3 parameters: 183767 + 1812 = 185579 doubles per system, 371158 per frequency -> 361 of 400
  CHECK(noisesens_work_doubles(302, 3) == 185579);
  CHECK(noisesens_freq_chunk(302, 3, 2, 400) == 361);
  CHECK((size_t)361 * 2 * 185579 <= DENSE_WORK_CAP && (size_t)362 * 2 * 185579 > DENSE_WORK_CAP);
  // its y-only launch: 183767 per system -> 365 frequencies
  CHECK(noisesens_freq_chunk(302, 0, 2, 400) == 365);
  CHECK(noisesens_freq_chunk(97, 1, 1, 7) == 7);                               // everything fits: all frequencies at once
  // exactly at the cap: one system of `per` doubles per frequency takes floor(2^27 / per) frequencies; one more double and it is one fewer
  const size_t per = noisesens_work_doubles(4096, 32);                         // 33835008
  CHECK(per == 33835008);
  CHECK(noisesens_freq_chunk(4096, 32, 1, 61) == (int)(DENSE_WORK_CAP / per) && DENSE_WORK_CAP / per == 3);
  CHECK(noisesens_freq_chunk(4096, 32, 4, 61) == 1 && noisesens_freq_chunk(4096, 32, 8, 61) == 1);   // never below 1
  CHECK(dense_work_chunk(DENSE_WORK_CAP / 4, 1, 9) == 4 && dense_work_chunk(DENSE_WORK_CAP / 4 + 1, 1, 9) == 3);
}

static void extra_row() {
  const int row = 3;
  const std::vector<double> t = {1, 2, 3, 4, 5, 6, 7, 8, 9};                   // three classes
  const std::vector<double> a = noisesens_npar_extra_row(t, 3, row, 1);
  CHECK(a.size() == 12);
  for (int i = 0; i < 9; ++i) CHECK(a[i] == t[i]);                             // the rows of the classes stay
  CHECK(a[9] == 4 && a[10] == 5 && a[11] == 6);                                // class 3 = a copy of class 1
  const std::vector<double> b = noisesens_npar_extra_row(t, 3, row, 2);
  CHECK(b.size() == 12 && b[9] == 7 && b[11] == 9);
  const std::vector<double> one = noisesens_npar_extra_row({1.5, 2.5}, 1, 2, 0);
  CHECK(one.size() == 4 && one[2] == 1.5 && one[3] == 2.5);
  const std::vector<double> padded = noisesens_npar_extra_row({1, 2, 3, 4, 0, 0}, 2, 2, 0);   // a table longer than its classes: the tail is dropped
  CHECK(padded.size() == 6 && padded[4] == 1 && padded[5] == 2);
  CHECK(noisesens_npar_extra_row(t, 3, row, 3).empty() && noisesens_npar_extra_row(t, 3, row, -1).empty());   // no such class
  CHECK(noisesens_npar_extra_row(t, 4, row, 0).empty() && noisesens_npar_extra_row(t, 0, row, 0).empty());    // a table too short, no classes
}

int main() {
  panels_and_workspace();
  chunk_rule();
  extra_row();
  std::printf("noisesens host: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
