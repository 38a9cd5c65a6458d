// Host-only test of the HIP-free parts of the transient and DC drivers (cedarsim.jl_amd/csrc/ch_stepper_host.hpp, ch_dc_start.hpp):
// resolve_tran_plan, persist_max_rows, collect_breakpoints, add_newton_iters and the restart passes of DcRestarts, each against the
// rule it replaced, written out here as tran_solve, tran_persistent, persist_consts and dc_solve had it, bit for bit.  Built with
// sanitizers by tests/test_host_tran_plan.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ch_dc_start.hpp"
#include "ch_stepper_host.hpp"

using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { if (nbad < 40) std::printf("line %d (%s): %s\n", __LINE__, g_what, #c); ++nbad; } } while (0)
static const char* g_what = "";
static int n_singular_seen = 0, n_donor_seen = 0;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }
static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

// ---- the option defaults as tran_solve had them ----
static void plan_defaults() {
  g_what = "resolve_tran_plan";
  const double spans[3][2] = {{0.0, 1e-6}, {2.5e-9, 7.75e-7}, {-1.0, 3.0}};
  for (const auto& sp : spans) for (double dtmin : {0.0, 3e-13}) for (double dtmax : {0.0, 2e-8}) for (int max_steps : {0, 77}) for (int nmax : {0, 4}) for (int order : {0, 1, 5, 9}) {
    ch_tran_opts o; std::memset(&o, 0, sizeof(o));
    o.dtmin = dtmin; o.dtmax = dtmax; o.max_steps = max_steps; o.newton_maxiters = nmax; o.max_order = order; o.dt0 = 1e-12;
    const double t0 = sp[0], t1 = sp[1];
    const int kmax = std::min(5, std::max(1, o.max_order));
    const double span = t1 - t0;
    const double dtmax_w = o.dtmax > 0 ? o.dtmax : span / 10.0, dtmin_w = o.dtmin > 0 ? o.dtmin : 1e-15 * span;
    const int max_steps_w = o.max_steps > 0 ? o.max_steps : 100000, nmaxit_w = o.newton_maxiters > 0 ? o.newton_maxiters : 10;
    const TranPlan p = resolve_tran_plan(t0, t1, o);
    CHECK(same_bits(p.t0, t0) && same_bits(p.t1, t1) && p.o == &o);
    CHECK(p.kmax == kmax); CHECK(same_bits(p.dtmax, dtmax_w)); CHECK(same_bits(p.dtmin, dtmin_w));
    CHECK(p.max_steps == max_steps_w); CHECK(p.nmaxit == nmaxit_w);
    CHECK(p.bps.empty() && p.bpc.empty());
    // the controller built from the plan is the one built from the eight values
    TranPlan q = p; q.bps = {0.5 * (t0 + t1), t1}; q.bpc = {1e-9, -1.0};
    StepControl a(q), b(t0, t1, o.dt0, dtmin_w, dtmax_w, kmax, q.bps, q.bpc);
    CHECK(same_bits(a.t, b.t) && same_bits(a.h, b.h) && same_bits(a.t1, b.t1) && same_bits(a.dtmin, b.dtmin) && same_bits(a.dtmax, b.dtmax) && a.kmax == b.kmax && &a.bps == &q.bps && &a.bpc == &q.bpc);
  }
}

// ---- the row count of the device stepper's output buffer as tran_persistent had it ----
static void max_rows() {
  g_what = "persist_max_rows";
  for (int n_saveat : {0, 1, 7}) for (int max_steps : {1, 1000, 100000}) for (size_t row_d : {(size_t)1, (size_t)64, (size_t)65536, (size_t)1 << 26}) for (long forced_v : {-1L, 0L, 1L, 100L, 5000000L}) for (int with : {0, 1}) {
    long long want;
    if (n_saveat > 0) want = (long long)n_saveat + 1;
    else want = std::min<long long>((long long)max_steps + 2, std::max<long long>(1024, std::min<long long>(1 << 20, (long long)((256u << 20) / (row_d * sizeof(double))))));
    if (n_saveat == 0 && with) want = std::max(2L, forced_v);
    const long long got = persist_max_rows(n_saveat, max_steps, row_d, with ? &forced_v : nullptr);
    CHECK(got == want); CHECK(got >= 2);
  }
}

// ---- break points: the two loops of tran_solve (every source of every parameter set) and of persist_consts (a workgroup's sources) ----
static std::vector<HSource> sources() {
  std::vector<HSource> src(4);
  for (HSource& s : src) { s.kind = CH_SRC_DC; s.dc = 0.0; for (double& p : s.par) p = 0.0; }
  src[0].kind = CH_SRC_PWL; src[0].ts = {0.0, 1e-7, 1e-7, 3e-7, 4.5e-7, 9e-7}; src[0].ys = {0.0, 0.0, 1.0, 1.0, 0.25, 0.25};   // a jump at 1e-7, corners behind it
  src[1].kind = CH_SRC_PULSE;   // periodic: v0 v1 td tr tf pw per
  src[2].kind = CH_SRC_SIN;     // vo va f td theta phase ncycles
  src[3].par[0] = 1.8;          // DC: no break points
  return src;
}
static std::vector<double> source_params(int n_sets) {
  std::vector<double> par((size_t)n_sets * 4 * CH_SRC_NPAR, 0.0);
  for (int s = 0; s < n_sets; ++s) {
    double* p1 = &par[((size_t)s * 4 + 1) * CH_SRC_NPAR]; double* p2 = &par[((size_t)s * 4 + 2) * CH_SRC_NPAR]; double* p3 = &par[((size_t)s * 4 + 3) * CH_SRC_NPAR];
    p1[0] = 0.0; p1[1] = 5.0; p1[2] = 2e-8 * (1 + s); p1[3] = 1e-8; p1[4] = 1.5e-8; p1[5] = 6e-8; p1[6] = 2.5e-7;
    p2[0] = 0.5; p2[1] = 0.4; p2[2] = 1e7 * (1 + 0.5 * s); p2[3] = 5e-8 * (1 + s); p2[4] = 0.0; p2[5] = 0.0; p2[6] = 4.0;
    p3[0] = 1.8;
  }
  return par;
}
static void breakpoints() {
  g_what = "collect_breakpoints";
  const std::vector<HSource> src = sources();
  const int nsrc = (int)src.size();
  const double spans[2][2] = {{0.0, 1e-6}, {1e-7, 6.2e-7}};
  for (int n_sets : {1, 3}) for (const auto& sp : spans) {
    const std::vector<double> par = source_params(n_sets);
    const double t0 = sp[0], t1 = sp[1];
    std::vector<double> bps_w, bpc_w, bps, bpc;
    { std::vector<std::pair<double, double>> pts;
      for (int s = 0; s < n_sets; ++s) for (int i = 0; i < nsrc; ++i) source_breakpoint_codes(src[i], &par[((size_t)s * nsrc + i) * CH_SRC_NPAR], t0, t1, pts);
      merge_breakpoints(pts, t1, bps_w, bpc_w); }
    collect_breakpoints(src, par, n_sets, t0, t1, bps, bpc);
    CHECK(same_bits(bps, bps_w)); CHECK(same_bits(bpc, bpc_w)); CHECK(bps.size() > 4 && bps.back() == t1 && bpc.back() < 0);
    // a workgroup's list: the sources its blocks need, first parameter set
    for (const std::vector<int>& need : {std::vector<int>{0}, std::vector<int>{1, 2}, std::vector<int>{0, 2, 3}, std::vector<int>{}}) {
      std::vector<double> wb_w, wc_w, wb, wc;
      { std::vector<std::pair<double, double>> pts;
        for (int i : need) source_breakpoint_codes(src[i], &par[(size_t)i * CH_SRC_NPAR], t0, t1, pts);
        merge_breakpoints(pts, t1, wb_w, wc_w); }
      collect_breakpoints(src, par, 1, t0, t1, wb, wc, &need);
      CHECK(same_bits(wb, wb_w)); CHECK(same_bits(wc, wc_w)); CHECK(!wb.empty() && wb.back() == t1);
    }
  }
}

// ---- the five-counter update as the four sites had it ----
static void newton_iters() {
  g_what = "add_newton_iters";
  ch_stats a, b; std::memset(&a, 0, sizeof(a)); std::memset(&b, 0, sizeof(b));
  a.nf = b.nf = 3; a.nreject = b.nreject = 2;
  for (long long n : {0LL, 7LL, 123456789012LL}) {
    const long long blk = 3 * n + 1;
    a.n_block_iters += blk; a.nnonliniter += n; a.nf += n; a.njacs += n; a.nfactors += n; a.nsolve += n;
    add_newton_iters(b, n, blk);
    CHECK(std::memcmp(&a, &b, sizeof(a)) == 0);
  }
}

// ---- the restart passes as dc_solve had them: its loop body between the download and the upload, and its harvest ----
struct OldPasses {
  int n_comp, S, n_unk, n_mna, n_active;
  std::vector<int> comp_uofs, comp_nc, unk_mna;
  std::vector<unsigned char> active, donor_ok; std::vector<Rng> rngs; std::vector<double> xs, xm; std::vector<int> bo;
  void guess(int r, bool homotopy, const double* x0) {
    auto block_of_unknown = [&](int u) { int c = (int)(std::upper_bound(comp_uofs.begin(), comp_uofs.end(), u) - comp_uofs.begin()) - 1; return c; };
    for (int s = 0; s < S; ++s) {
      bool any = false;
      for (int c = 0; c < n_comp; ++c) if (active[(size_t)c * S + s]) any = true;
      if (!any) continue;
      if (!homotopy) {
        if (r == 0 && x0) for (int i = 0; i < n_mna; ++i) xm[i] = x0[(size_t)s * n_mna + i];
        else for (int i = 0; i < n_mna; ++i) xm[i] = 1e-7 * rngs[s].normal();
      } else std::fill(xm.begin(), xm.end(), 0.0);
      for (int u = 0; u < n_unk; ++u) if (active[(size_t)block_of_unknown(u) * S + s]) xs[(size_t)s * n_unk + u] = xm[unk_mna[u]];
    }
    if (r == 1 && S > 1) {
      for (int c = 0; c < n_comp; ++c) {
        int donor = -1;
        for (int s = 0; s < S && donor < 0; ++s) if (!active[(size_t)c * S + s] && donor_ok[(size_t)c * S + s]) donor = s;
        if (donor < 0) continue;
        for (int s = 0; s < S; ++s) if (active[(size_t)c * S + s])
          for (int u = comp_uofs[c]; u < comp_uofs[c] + comp_nc[c]; ++u) xs[(size_t)s * n_unk + u] = xs[(size_t)donor * n_unk + u];
      }
    }
  }
  void harvest() {
    const int nblk = n_comp * S;
    n_active = 0;
    for (int b = 0; b < nblk; ++b) if (active[b]) { if (bo[b] == 0) { active[b] = 0; donor_ok[b] = 1; } else ++n_active; }
  }
  void status_out(std::vector<int>& out) const {
    const int nblk = n_comp * S;
    out.assign(S, CH_OK); for (int b = 0; b < nblk; ++b) if (active[b]) out[b % S] = bo[b] == 2 ? CH_ERR_SINGULAR : CH_ERR_MAXITERS;
  }
};
static void restart_passes() {
  g_what = "DcRestarts";
  for (int n_comp : {1, 3}) for (int S : {1, 3}) for (int with_x0 : {0, 1}) for (int with_donor : {0, 1}) {
    // blocks of 4, 3, 5 unknowns; 15 MNA entries, the map neither sorted nor contiguous
    Analysis A;
    A.n_comp = n_comp; A.n_mna = 15;
    const int ncs[3] = {4, 3, 5};
    for (int c = 0, u = 0; c < n_comp; ++c) { A.comp_uofs.push_back(u); A.comp_nc.push_back(ncs[c]); u += ncs[c]; A.n_unk = u; }
    for (int u = 0; u < A.n_unk; ++u) A.unk_mna.push_back((u * 7 + 3) % A.n_mna);
    const int nblk = n_comp * S;
    std::vector<double> x0((size_t)S * A.n_mna);
    for (size_t i = 0; i < x0.size(); ++i) x0[i] = 0.25 + 0.001 * (double)i;
    const uint64_t seed = 10;
    // with x0 the generators start at the seeds; without, behind the first pass' fill (the cached start)
    DcStart st; st.fill(seed, S, A.n_mna, A.unk_mna);
    const std::vector<Rng> start = with_x0 ? dc_start_rngs(seed, S) : st.after;
    OldPasses O{n_comp, S, A.n_unk, A.n_mna, nblk, A.comp_uofs, A.comp_nc, A.unk_mna, std::vector<unsigned char>(nblk, 1), std::vector<unsigned char>(nblk, 0),
                start, std::vector<double>((size_t)S * A.n_unk), std::vector<double>(A.n_mna), std::vector<int>(nblk, 0)};
    DcRestarts P(A, S, start);
    CHECK(P.n_active == nblk && P.nblk == nblk && P.xs.size() == O.xs.size());
    // what the ring slot held before: both sides start from the same state (the cached start, or a pattern)
    for (size_t i = 0; i < O.xs.size(); ++i) O.xs[i] = P.xs[i] = with_x0 ? -1.0 - (double)i : st.xs[i];
    const int nrest = 3;
    for (int r = 0; r <= nrest; ++r) {
      const bool homotopy = r == nrest;
      if (r > 0 || with_x0) {   // pass 0 without x0 is a copy on the device: no host guess
        O.guess(r, homotopy, with_x0 ? x0.data() : nullptr); P.guess(A, r, homotopy, with_x0 ? x0.data() : nullptr);
        CHECK(same_bits(P.xs, O.xs));
        for (int s = 0; s < S; ++s) CHECK(P.rngs[s].s == O.rngs[s].s);
      }
      // statuses of the pass: pass 0 converges (with_donor) every block of sample 0 and block 0 of every sample; pass 1 the
      // last sample's blocks; pass 2 nothing, one block singular; the homotopy pass everything but the singular block
      for (int c = 0; c < n_comp; ++c) for (int s = 0; s < S; ++s) {
        const int b = c * S + s;
        int stt = 1;
        if (r == 0 && with_donor && (s == 0 || c == 0)) stt = 0;
        if (r == 1 && s == S - 1) stt = 0;
        if (r == nrest) stt = 0;
        if (r >= 2 && c == n_comp - 1 && s == S / 2 && !(with_donor && (s == 0 || c == 0)) && s != S - 1) stt = 2;
        O.bo[b] = P.status[b] = stt;
      }
      O.harvest(); P.harvest();
      CHECK(P.n_active == O.n_active); CHECK(P.active == O.active); CHECK(P.donor_ok == O.donor_ok);
      std::vector<int> so, sp; O.status_out(so); P.sample_status(sp);
      CHECK(so == sp);
      for (int v : sp) if (v == CH_ERR_SINGULAR) ++n_singular_seen;
      if (r == 0 && S > 1 && with_donor && P.n_active > 0) ++n_donor_seen;
      if (P.n_active == 0) break;
    }
  }
}

int main() {
  plan_defaults(); max_rows(); breakpoints(); newton_iters(); restart_passes();
  g_what = "coverage"; CHECK(n_singular_seen > 0); CHECK(n_donor_seen > 0);   // a singular block was harvested; a donor pass ran
  std::printf("tran plan: %d checks, %d bad\n", nchecked, nbad);
  return nbad == 0 ? 0 : 1;
}
