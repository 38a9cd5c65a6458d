// ch_sparse_newton.hpp — the Newton policy of the sparse path (pure C++, no HIP): every per-sample decision that
// ch_circuit::run_sparse (ch_engine_sparse.hpp) takes between its launches, from the plain numbers the kernels of ch_sparse.hpp
// leave in mapped host memory.  It is the rule the fused kernels of ch_kernels.hpp implement inside one launch: DC residual test,
// uniform voltage limiting, IDA's convergence-rate test on the first iteration of a time step, the ageing of the rate, one
// re-analysis after a failed static pivot.  Kept free of device code so that the CPU test-suite can drive it with scripted numbers
// (tests/host_sparse_newton.cpp, under the sanitizers of tests/test_host_analysis_fuzz.py).
//
//   red   [S][8] doubles per sample: {0 ‖F‖inf, 1 max|dx|, 2 Σ(w dx)², 3 -, 4..6 local-error sums of orders k, k-1, k+1, 7 their count}
//   flag  [S][2] ints per sample:    {0 the factorisation met a zero / non-finite pivot, 1 the update produced a non-finite value}
//   status 0 converged, 1 not converged, 2 singular / non-finite (BlockOut::status)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace chip {

struct SparseNewton {
  struct Solve {   // what one solve takes from the launch arguments
    bool dc = false, tran = false, reset_rate = false;   // neither dc nor tran: evaluation only
    int n = 0;                                           // unknowns (the WRMS norm divides by it)
    double newton_tol = 0.0, dc_abstol = 0.0, dv_max = 0.0;
  };
  enum class Factored { DONE, REANALYSE, SINGULAR };

  // ---- across solves ----
  int S = 0;
  std::vector<double> rate_v;   // per sample: Newton convergence rate seen by the last converged time step
  std::vector<int> status_v;    // per sample: status of the last solve it took part in
  // ---- one solve ----
  Solve cfg;
  std::vector<int> todo;        // samples taking part in this solve
  std::vector<int> act;         // ... still iterating
  std::vector<int> work;        // ... whose factorisation is still to be done in this iteration
  std::vector<int> failed;      // ... whose last factorisation met a bad pivot
  std::vector<int> status, iters;
  std::vector<double> rate_prev, rate_new, dn_prev, fnorm, scale;

  void reset(int n_samples) { S = n_samples; rate_v.assign(S, 1.0); status_v.assign(S, 0); }

  // a sample takes part when any of its blocks is active (the sparse system spans all blocks); host_active: [n_comp][S] or null
  void begin(const Solve& c, const unsigned char* host_active, int n_comp) {
    cfg = c;
    todo.clear();
    for (int sm = 0; sm < S; ++sm) {
      bool on = !host_active;
      for (int k = 0; k < n_comp && !on; ++k) on = host_active[(size_t)k * S + sm] != 0;
      if (on) todo.push_back(sm);
    }
    status.assign(S, 1); iters.assign(S, 0);
    rate_prev.assign(S, 1.0); rate_new.assign(S, -1.0); dn_prev.assign(S, 0.0); fnorm.assign(S, 0.0); scale.assign(S, 1.0);
    for (int sm : todo) rate_prev[sm] = (cfg.tran && !cfg.reset_rate) ? rate_v[sm] : 1.0;
    act = todo; work.clear(); failed.clear();
  }
  void accept_all() { for (int sm : act) status[sm] = 0; }                  // evaluation only: nothing to converge
  void drop_all_singular() { for (int sm : act) status[sm] = 2; act.clear(); }   // no plan could be made

  // DC, after the residual pass: converged, singular (NaN or > 1e300), or continue.  True when the active list changed.
  bool dc_residual(const double* red) {
    keep_.clear();
    for (int sm : act) {
      fnorm[sm] = red[(size_t)sm * 8];
      if (!(fnorm[sm] == fnorm[sm]) || fnorm[sm] > 1e300) status[sm] = 2;
      else if (fnorm[sm] < cfg.dc_abstol) status[sm] = 0;
      else keep_.push_back(sm);
    }
    return shrink_();
  }

  void begin_factor() { work = act; }
  // uniform voltage limiting of the samples of `work`: dv_max / max|dx| only where the factorisation succeeded and the step is longer
  void limit_steps(const double* red, const int* flag) {
    for (int sm : work) {
      scale[sm] = 1.0;
      const double mx = red[(size_t)sm * 8 + 1];
      if (!flag[(size_t)sm * 2] && mx > cfg.dv_max) scale[sm] = cfg.dv_max / mx;
    }
  }
  // After the factorisation + update of `work`.  A static pivot became zero: re-analyse once with the current values of the
  // first failing sample (KLU would re-pivot here too) and redo the failing samples — the others have already taken their step;
  // on a plan made in this iteration, or on the second attempt, the failing samples are singular.
  Factored after_factor(const int* flag, bool fresh_plan, int attempt) {
    failed.clear();
    for (int sm : work) if (flag[(size_t)sm * 2]) failed.push_back(sm);
    if (failed.empty()) return Factored::DONE;
    if (fresh_plan || attempt == 1) { drop_failed(); work.clear(); return Factored::SINGULAR; }
    return Factored::REANALYSE;
  }
  void drop_failed() {
    for (int sm : failed) status[sm] = 2;
    act.erase(std::remove_if(act.begin(), act.end(), [&](int q) { return status[q] == 2; }), act.end());
  }
  void retry_failed() { work.swap(failed); }

  // After the update of iteration `it`: one more iteration counted, non-finite update = singular, and in a time step the
  // convergence test on ‖dx‖ (WRMS) — on the first iteration also IDA's estimate from the rate of the previous step.  True when the
  // active list changed.
  bool after_update(int it, const double* red, const int* flag) {
    keep_.clear();
    for (int sm : act) {
      if (status[sm] == 2) continue;
      ++iters[sm];
      if (flag[(size_t)sm * 2 + 1]) { status[sm] = 2; continue; }
      if (cfg.tran) {
        const double dn = std::sqrt(red[(size_t)sm * 8 + 2] / cfg.n);
        bool conv = false;
        if (it == 0) conv = dn <= cfg.newton_tol || (rate_prev[sm] < 0.9 && 2.0 * std::max(rate_prev[sm], 0.02) * dn <= cfg.newton_tol);
        else { rate_new[sm] = dn_prev[sm] > 0 ? dn / dn_prev[sm] : 0.0; conv = dn <= cfg.newton_tol; }
        dn_prev[sm] = dn;
        if (conv) { status[sm] = 0; continue; }
      }
      keep_.push_back(sm);
    }
    return shrink_();
  }

  // end of the iterations: the rate a converged time step leaves behind — measured when it took two iterations or more, aged otherwise
  void end_iterations() {
    for (int sm : todo)
      if (cfg.tran && status[sm] == 0) rate_v[sm] = iters[sm] >= 2 ? std::min(1.0, std::max(rate_new[sm], 1e-4)) : std::min(1.0, rate_prev[sm] * 1.5);
  }
  // after the commit pass: status_v and the fields of Summary (ch_kernels.hpp; a template so that this header needs no HIP);
  // ck, ckm1, ckp1: error constants of orders k, k-1, k+1
  template <class Sum>
  void summarise(Sum& out, const double* red, double ck, double ckm1, double ckp1) {
    for (int sm : todo) {
      status_v[sm] = status[sm];
      if (status[sm] != 0) ++out.n_fail;
      if (status[sm] == 2) ++out.n_singular;
      out.max_iters = std::max(out.max_iters, iters[sm]); out.sum_iters += iters[sm]; out.sum_block_iters += iters[sm]; out.fnorm = std::max(out.fnorm, fnorm[sm]);
      const double* r = red + (size_t)sm * 8;
      if (cfg.tran && r[7] > 0) {
        out.errk = std::max(out.errk, ck * std::sqrt(r[4] / r[7])); out.errkm1 = std::max(out.errkm1, ckm1 * std::sqrt(r[5] / r[7])); out.errkp1 = std::max(out.errkp1, ckp1 * std::sqrt(r[6] / r[7]));
      }
    }
  }

 private:
  std::vector<int> keep_;
  bool shrink_() { if (keep_.size() == act.size()) return false; act.swap(keep_); return true; }
};

}  // namespace chip
