// Host-only test of the sparse path's Newton policy (cedarsim.jl_amd/csrc/ch_sparse_newton.hpp): the object is driven with scripted
// reduction numbers and flags, in the order ch_circuit::run_sparse calls it, and every decision is compared with what the rule says
// — worked out by hand in the comments, never taken from the code under test.  Numbers are chosen so that every square root and
// quotient is exact in binary.  Built with sanitizers by tests/test_host_analysis_fuzz.py.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "ch_sparse_newton.hpp"
using namespace chip;
using F = SparseNewton::Factored;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); ++nbad; } } while (0)
using VI = std::vector<int>;

struct Sum { int n_fail = 0, max_iters = 0, n_singular = 0, pad = 0; long long sum_iters = 0, sum_block_iters = 0; double errk = 0, errkm1 = 0, errkp1 = 0, fnorm = 0; };
struct Host {   // the mapped reductions and flags
  std::vector<double> red; std::vector<int> flag;
  explicit Host(int S) : red((size_t)S * 8, 0.0), flag((size_t)S * 2, 0) {}
  double& r(int sm, int k) { return red[(size_t)sm * 8 + k]; }
  int& f(int sm, int k) { return flag[(size_t)sm * 2 + k]; }
  void dn(int sm, double v, int n) { r(sm, 2) = v * v * n; }   // the update pass leaves sum (w dx)^2; the policy takes sqrt(sum / n)
};

// ---- operating point: residual test, voltage limiting, maxit ----
static void dc_solve() {
  const int S = 5;   // maxit = 2
  SparseNewton nw; nw.reset(S);
  SparseNewton::Solve c; c.dc = true; c.n = 4; c.dc_abstol = 1e-9; c.dv_max = 2.0; c.newton_tol = 0.25;
  Host h(S);
  nw.begin(c, nullptr, 3);
  CHECK(nw.todo == (VI{0, 1, 2, 3, 4}) && nw.act == nw.todo);
  // it 0 — ‖F‖: 5e-10 < 1e-9 converged | NaN singular | 1.0 continue | 2e300 > 1e300 singular | exactly the tolerance: not below it, continue
  h.r(0, 0) = 5e-10; h.r(1, 0) = std::numeric_limits<double>::quiet_NaN(); h.r(2, 0) = 1.0; h.r(3, 0) = 2e300; h.r(4, 0) = 1e-9;
  CHECK(nw.dc_residual(h.red.data()) == true);
  CHECK(nw.act == (VI{2, 4}));
  CHECK(nw.status == (VI{0, 2, 1, 2, 1}));
  nw.begin_factor();
  CHECK(nw.work == (VI{2, 4}));
  // max|dx| 8 with dv_max 2: scale 1/4; exactly dv_max: not above it, 1
  h.r(2, 1) = 8.0; h.r(4, 1) = 2.0;
  nw.limit_steps(h.red.data(), h.flag.data());
  CHECK(nw.scale[2] == 0.25 && nw.scale[4] == 1.0);
  // a flagged factorisation is never scaled, however long its (meaningless) step; an earlier scale does not survive
  h.f(2, 0) = 1; h.r(4, 1) = 1.0;
  nw.limit_steps(h.red.data(), h.flag.data());
  CHECK(nw.scale[2] == 1.0 && nw.scale[4] == 1.0);
  h.f(2, 0) = 0;
  CHECK(nw.after_factor(h.flag.data(), true, 0) == F::DONE);
  CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == false);   // no test on dx at the operating point: both go on
  CHECK(nw.act == (VI{2, 4}) && nw.iters == (VI{0, 0, 1, 0, 1}));
  // it 1 — sample 4 converges, sample 2 goes on
  h.r(2, 0) = 0.5; h.r(4, 0) = 1e-12;
  CHECK(nw.dc_residual(h.red.data()) == true && nw.act == (VI{2}));
  nw.begin_factor();
  CHECK(nw.after_factor(h.flag.data(), false, 0) == F::DONE);
  CHECK(nw.after_update(1, h.red.data(), h.flag.data()) == false);
  // it 2 == maxit — the residual is still tested, then the loop ends: sample 2 has not converged after two iterations
  h.r(2, 0) = 0.25;
  CHECK(nw.dc_residual(h.red.data()) == false && nw.act == (VI{2}));
  nw.end_iterations();
  Sum out;
  nw.summarise(out, h.red.data(), 1.0, 1.0, 1.0);
  CHECK(nw.status_v == (VI{0, 2, 1, 2, 0}));
  CHECK(out.n_fail == 3 && out.n_singular == 2 && out.max_iters == 2 && out.sum_iters == 3 && out.sum_block_iters == 3);
  CHECK(out.fnorm == 2e300);                        // the largest residual seen; a NaN never wins a comparison
  CHECK(out.errk == 0.0 && out.errkm1 == 0.0 && out.errkp1 == 0.0);   // no local error at the operating point
  for (double r : nw.rate_v) CHECK(r == 1.0);       // and no rate
}

// ---- time step, first iteration: dn <= tol, or rate_prev < 0.9 and 2 max(rate_prev, 0.02) dn <= tol ----
static void first_iteration_acceptance() {
  const int S = 8, n = 4;
  SparseNewton nw; nw.reset(S);
  SparseNewton::Solve c; c.tran = true; c.n = n; c.newton_tol = 0.25;
  Host h(S);
  //          rate     dn      2 max(rate, .02) dn
  // 0        0.25     0.5     0.25  = tol            accept
  // 1        0.26     0.5     0.26  > tol            go on
  // 2        0.001    6       0.24  (floor 0.02)     accept
  // 3        0.001    6.5     0.26  (floor 0.02)     go on
  // 4        0.89     0.125   dn <= tol on its own   accept
  // 5        0.9      0.25    dn = tol on its own    accept
  // 6        0.9      0.5     rate not below 0.9     go on
  // 7        0.89     0.5     0.89  > tol            go on     (from 0.5 upwards the estimate never decides alone)
  const double rate[S] = {0.25, 0.26, 0.001, 0.001, 0.89, 0.9, 0.9, 0.89}, dn[S] = {0.5, 0.5, 6.0, 6.5, 0.125, 0.25, 0.5, 0.5};
  for (int s = 0; s < S; ++s) { nw.rate_v[s] = rate[s]; h.dn(s, dn[s], n); }
  nw.begin(c, nullptr, 1);
  nw.begin_factor();
  CHECK(nw.after_factor(h.flag.data(), false, 0) == F::DONE);
  CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == true);
  CHECK(nw.act == (VI{1, 3, 6, 7}));
  CHECK(nw.status == (VI{0, 1, 0, 1, 0, 0, 1, 1}));
  // reset_rate: every stored rate is ignored (1.0), only dn <= tol accepts
  c.reset_rate = true;
  nw.begin(c, nullptr, 1);
  for (int s = 0; s < S; ++s) CHECK(nw.rate_prev[s] == 1.0);
  nw.begin_factor();
  CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == true);
  CHECK(nw.act == (VI{0, 1, 2, 3, 6, 7}));
  // a one-iteration step ages the rate by 1.5, capped at 1 — from the rate the solve STARTED with (1.0 after the reset)
  nw.end_iterations();
  CHECK(nw.rate_v[4] == 1.0 && nw.rate_v[5] == 1.0 && nw.rate_v[0] == 0.25);   // sample 0 did not converge: untouched
}

// ---- the rate a converged step leaves behind ----
static void rate_refresh_and_ageing() {
  const int S = 4, n = 4;
  SparseNewton nw; nw.reset(S);
  SparseNewton::Solve c; c.tran = true; c.n = n; c.newton_tol = 0.25;
  Host h(S);
  nw.rate_v = {1.0, 1.0, 0.5, 0.75};
  nw.begin(c, nullptr, 1);
  // it 0: samples 0, 1 far away (dn 4); samples 2, 3 converge at once (dn 0.125)
  h.dn(0, 4.0, n); h.dn(1, 4.0, n); h.dn(2, 0.125, n); h.dn(3, 0.125, n);
  nw.begin_factor();
  CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == true && nw.act == (VI{0, 1}));
  // it 1: dn 0.125 and 2^-14: rates 0.125 / 4 = 0.03125 and 2^-16 = 1.5e-5, the second below the floor 1e-4
  h.dn(0, 0.125, n); h.dn(1, std::ldexp(1.0, -14), n);
  nw.begin_factor();
  CHECK(nw.after_update(1, h.red.data(), h.flag.data()) == true && nw.act.empty());
  nw.end_iterations();
  CHECK(nw.iters == (VI{2, 2, 1, 1}));
  CHECK(nw.rate_v[0] == 0.03125 && nw.rate_v[1] == 1e-4);
  // (a step that converges in two iterations or more has dn falling from above tol to below it: its measured rate is below 1, the
  //  upper clamp of the refreshed rate cannot be reached from outside)
  CHECK(nw.rate_v[2] == 0.75);   // one iteration: 0.5 * 1.5
  CHECK(nw.rate_v[3] == 1.0);    // 0.75 * 1.5 = 1.125, capped
  // a non-finite update is singular whatever dn says, and leaves the rate alone
  nw.begin(c, nullptr, 1);
  h.f(2, 1) = 1;
  nw.begin_factor();
  CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == true);
  CHECK(nw.status[2] == 2 && nw.iters[2] == 1);
  nw.end_iterations();
  CHECK(nw.rate_v[2] == 0.75);
}

// ---- a static pivot fails ----
static void failed_pivots() {
  const int S = 4;
  SparseNewton::Solve c; c.dc = true; c.n = 4; c.dc_abstol = 1e-9; c.dv_max = 0.0;
  { // reused plan, first attempt: re-analyse with the first failing sample, redo only the failing ones; the second attempt succeeds
    SparseNewton nw; nw.reset(S); Host h(S);
    for (int s = 0; s < S; ++s) h.r(s, 0) = 1.0;
    nw.begin(c, nullptr, 1);
    CHECK(nw.dc_residual(h.red.data()) == false);
    nw.begin_factor();
    h.f(1, 0) = 1; h.f(3, 0) = 1;
    CHECK(nw.after_factor(h.flag.data(), false, 0) == F::REANALYSE);
    CHECK(nw.failed == (VI{1, 3}) && nw.failed[0] == 1);
    CHECK(nw.act == (VI{0, 1, 2, 3}) && nw.status == (VI{1, 1, 1, 1}));   // nobody dropped yet
    nw.retry_failed();
    CHECK(nw.work == (VI{1, 3}));
    h.f(1, 0) = 0; h.f(3, 0) = 0;
    CHECK(nw.after_factor(h.flag.data(), true, 1) == F::DONE);
    CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == false);
    CHECK(nw.iters == (VI{1, 1, 1, 1}) && nw.act == (VI{0, 1, 2, 3}));
  }
  { // ... the second attempt fails for sample 3: singular, the others keep their step
    SparseNewton nw; nw.reset(S); Host h(S);
    for (int s = 0; s < S; ++s) h.r(s, 0) = 1.0;
    nw.begin(c, nullptr, 1);
    nw.dc_residual(h.red.data());
    nw.begin_factor();
    h.f(1, 0) = 1; h.f(3, 0) = 1;
    CHECK(nw.after_factor(h.flag.data(), false, 0) == F::REANALYSE);
    nw.retry_failed();
    h.f(1, 0) = 0;
    CHECK(nw.after_factor(h.flag.data(), true, 1) == F::SINGULAR);
    CHECK(nw.status == (VI{1, 1, 1, 2}) && nw.act == (VI{0, 1, 2}) && nw.work.empty());
    nw.after_update(0, h.red.data(), h.flag.data());
    CHECK(nw.iters == (VI{1, 1, 1, 0}) && nw.act == (VI{0, 1, 2}));
    Sum out; nw.end_iterations(); nw.summarise(out, h.red.data(), 1.0, 1.0, 1.0);
    CHECK(out.n_fail == 4 && out.n_singular == 1 && out.max_iters == 1 && out.sum_iters == 3);
  }
  { // a plan made in this very iteration: no second analysis, singular at once
    SparseNewton nw; nw.reset(S); Host h(S);
    for (int s = 0; s < S; ++s) h.r(s, 0) = 1.0;
    nw.begin(c, nullptr, 1);
    nw.dc_residual(h.red.data());
    nw.begin_factor();
    h.f(0, 0) = 1;
    CHECK(nw.after_factor(h.flag.data(), true, 0) == F::SINGULAR);
    CHECK(nw.status == (VI{2, 1, 1, 1}) && nw.act == (VI{1, 2, 3}) && nw.work.empty());
    nw.after_update(0, h.red.data(), h.flag.data());
    CHECK(nw.iters == (VI{0, 1, 1, 1}));
  }
  { // the re-analysis itself fails (structurally singular): the caller drops the failing samples; no plan at all: everybody
    SparseNewton nw; nw.reset(S); Host h(S);
    for (int s = 0; s < S; ++s) h.r(s, 0) = 1.0;
    nw.begin(c, nullptr, 1);
    nw.dc_residual(h.red.data());
    nw.begin_factor();
    h.f(2, 0) = 1;
    CHECK(nw.after_factor(h.flag.data(), false, 0) == F::REANALYSE);
    nw.drop_failed();
    CHECK(nw.status == (VI{1, 1, 2, 1}) && nw.act == (VI{0, 1, 3}));
    nw.drop_all_singular();
    CHECK(nw.status == (VI{2, 2, 2, 2}) && nw.act.empty());
  }
}

// ---- a batch whose samples finish at different iterations; one sample switched off by the active mask ----
static void shrinking_batch() {
  const int S = 4, n = 4, n_comp = 2;
  SparseNewton nw; nw.reset(S);
  nw.status_v[3] = 7;
  SparseNewton::Solve c; c.tran = true; c.reset_rate = true; c.n = n; c.newton_tol = 0.25;
  // [n_comp][S]: sample 0 active in both blocks, sample 1 in the first, sample 2 in the second only, sample 3 in none
  const unsigned char active[n_comp * S] = {1, 1, 0, 0, 1, 0, 1, 0};
  Host h(S);
  nw.begin(c, active, n_comp);
  CHECK(nw.todo == (VI{0, 1, 2}) && nw.act == nw.todo);
  h.dn(0, 0.125, n); h.dn(1, 4.0, n); h.dn(2, 4.0, n); h.dn(3, 0.0, n);
  nw.begin_factor();
  CHECK(nw.after_factor(h.flag.data(), false, 0) == F::DONE);
  CHECK(nw.after_update(0, h.red.data(), h.flag.data()) == true && nw.act == (VI{1, 2}));
  h.dn(1, 0.125, n); h.dn(2, 1.0, n);
  nw.begin_factor();
  CHECK(nw.work == (VI{1, 2}));
  CHECK(nw.after_update(1, h.red.data(), h.flag.data()) == true && nw.act == (VI{2}));
  h.dn(2, 0.125, n);
  nw.begin_factor();
  CHECK(nw.after_update(2, h.red.data(), h.flag.data()) == true && nw.act.empty());
  nw.end_iterations();
  CHECK(nw.iters == (VI{1, 2, 3, 0}));
  // rates: one iteration from 1.0 (reset): min(1, 1.5) = 1; 0.125 / 4; 0.125 / 1
  CHECK(nw.rate_v[0] == 1.0 && nw.rate_v[1] == 0.03125 && nw.rate_v[2] == 0.125 && nw.rate_v[3] == 1.0);
  // commit sums {e_k, e_k-1, e_k+1, count}: sample 0 {16, 4, 64, 4}, sample 1 no differential unknown (count 0: skipped), sample 2 {36, 1, 256, 4}
  // errk   = 0.5  max(sqrt(16/4), sqrt(36/4))  = 0.5 * 3  = 1.5
  // errkm1 = 2    max(sqrt(4/4),  sqrt(1/4))   = 2 * 1    = 2
  // errkp1 = 0.25 max(sqrt(64/4), sqrt(256/4)) = 0.25 * 8 = 2
  const double sums[3][4] = {{16, 4, 64, 4}, {1e6, 1e6, 1e6, 0}, {36, 1, 256, 4}};
  for (int s = 0; s < 3; ++s) for (int k = 0; k < 4; ++k) h.r(s, 4 + k) = sums[s][k];
  h.r(3, 4) = 1e12; h.r(3, 7) = 1.0;   // not part of the solve: never read
  Sum out;
  nw.summarise(out, h.red.data(), 0.5, 2.0, 0.25);
  CHECK(out.n_fail == 0 && out.n_singular == 0 && out.max_iters == 3 && out.sum_iters == 6 && out.sum_block_iters == 6);
  CHECK(out.errk == 1.5 && out.errkm1 == 2.0 && out.errkp1 == 2.0 && out.fnorm == 0.0);
  CHECK(nw.status_v == (VI{0, 0, 0, 7}));
  // evaluation only (neither dc nor tran): everybody accepted without an iteration
  SparseNewton::Solve ev; ev.n = n;
  nw.begin(ev, nullptr, n_comp);
  nw.accept_all();
  Sum o2; nw.end_iterations(); nw.summarise(o2, h.red.data(), 0.5, 2.0, 0.25);
  CHECK(o2.n_fail == 0 && o2.max_iters == 0 && o2.errk == 0.0 && nw.status_v == (VI{0, 0, 0, 0}));
  // nobody active: nothing to do
  const unsigned char none[n_comp * S] = {0, 0, 0, 0, 0, 0, 0, 0};
  nw.begin(c, none, n_comp);
  CHECK(nw.todo.empty() && nw.act.empty());
}

int main() {
  dc_solve();
  first_iteration_acceptance();
  rate_refresh_and_ageing();
  failed_pivots();
  shrinking_batch();
  std::printf("sparse newton policy: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
