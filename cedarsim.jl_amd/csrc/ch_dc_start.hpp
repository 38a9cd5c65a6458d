// ch_dc_start.hpp — the random start of the DC operating point, HIP-free: the generator (u0 = 1e-7*randn, dcop.jl:60), the rule
// "MNA start -> unknown-space state", and the per-circuit cache of the first pass' start vector.  The numbers of the first pass
// are a pure function of (seed, S, n_mna) and of the circuit's unknown map, so a circuit draws them once: DcStart keeps the
// unknown-space start and every sample's generator state BEHIND that fill, from which the restarts go on drawing exactly the
// numbers they drew when every call started from the seed.  DcRestarts is the host side of the passes behind it: each pass' guess
// for the blocks still active (x0, fresh draws, a donor sample's state, zero for the gmin ladder) and the harvest of its statuses.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "ch_analysis.hpp"

namespace chip {

// ---- RNG: splitmix64 + Box-Muller, as specified for the DC initial guess u0 = 1e-7*randn (dcop.jl:60)
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uniform() { return ((next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
  double normal() { double u1 = uniform(), u2 = uniform(); return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2); }
};

// sample s of a batch draws from its own generator
inline std::vector<Rng> dc_start_rngs(uint64_t seed, int S) {
  std::vector<Rng> r; r.reserve((size_t)S);
  for (int s = 0; s < S; ++s) r.emplace_back(seed + (uint64_t)s);
  return r;
}
// one sample's random MNA start: n_mna draws, in MNA order
inline void dc_random_mna(Rng& rng, std::vector<double>& xm) { for (double& v : xm) v = 1e-7 * rng.normal(); }
// MNA start -> the unknowns of one sample: unknown u takes the value of its representative MNA entry
inline void dc_mna_to_unknowns(const double* xm, const std::vector<int>& unk_mna, double* xs) {
  for (size_t u = 0; u < unk_mna.size(); ++u) xs[u] = xm[unk_mna[u]];
}

// The first pass of a DC solve that has no x0 (every block active): [S][n_unk] start and the generators behind it.
struct DcStart {
  bool valid = false; uint64_t seed = 0; int S = 0;
  std::vector<double> xs;      // unknown-space start, as the first pass writes it into the ring slot
  std::vector<Rng> after;      // every sample's generator after its n_mna draws: where the restarts continue
  bool matches(uint64_t sd, int s) const { return valid && seed == sd && S == s; }
  void fill(uint64_t sd, int s, int n_mna, const std::vector<int>& unk_mna) {
    seed = sd; S = s; valid = true;
    after = dc_start_rngs(sd, s);
    xs.assign((size_t)s * unk_mna.size(), 0.0);
    std::vector<double> xm((size_t)n_mna);
    for (int q = 0; q < s; ++q) { dc_random_mna(after[q], xm); dc_mna_to_unknowns(xm.data(), unk_mna, xs.data() + (size_t)q * unk_mna.size()); }
  }
};

// The restart passes of one DC solve, host side: which blocks [n_comp][S] are still active, which have converged in this call (a
// valid starting point for their siblings), every sample's generator, the blocks' statuses of the last pass (0 = converged,
// 2 = singular) and the slot's unknowns xs [S][n_unk] between their download and their upload.
struct DcRestarts {
  const int S, nblk; int n_active;
  std::vector<unsigned char> active, donor_ok;
  std::vector<Rng> rngs; std::vector<int> status; std::vector<double> xs, xm;
  DcRestarts(const Analysis& A, int S_, std::vector<Rng> rngs_)
      : S(S_), nblk(A.n_comp * S_), n_active(nblk), active(nblk, 1), donor_ok(nblk, 0), rngs(std::move(rngs_)), status(nblk, 0), xs((size_t)S_ * A.n_unk), xm(A.n_mna) {}
  // Initial guess of pass r for the active blocks, written over their unknowns in xs: x0 (pass 0), zero (the homotopy pass),
  // otherwise n_mna fresh draws per sample that has an active block.
  void guess(const Analysis& A, int r, bool homotopy, const double* x0) {
    auto block_of_unknown = [&](int u) { int c = (int)(std::upper_bound(A.comp_uofs.begin(), A.comp_uofs.end(), u) - A.comp_uofs.begin()) - 1; return c; };
    for (int s = 0; s < S; ++s) {
      bool any = false;
      for (int c = 0; c < A.n_comp; ++c) if (active[(size_t)c * S + s]) any = true;
      if (!any) continue;
      if (!homotopy) {
        if (r == 0 && x0) for (int i = 0; i < A.n_mna; ++i) xm[i] = x0[(size_t)s * A.n_mna + i];
        else for (int i = 0; i < A.n_mna; ++i) xm[i] = 1e-7 * rngs[s].normal();
      } else std::fill(xm.begin(), xm.end(), 0.0);
      for (int u = 0; u < A.n_unk; ++u) if (active[(size_t)block_of_unknown(u) * S + s]) xs[(size_t)s * A.n_unk + u] = xm[A.unk_mna[u]];
    }
    // First restart of a batch: a block that did not converge from the random start is started from the operating point of the
    // same block in a sample that did (continuation from a neighbouring parameter set) — a few iterations instead of another
    // `maxiters` spent from 1e-7*randn; later restarts are random again as in the reference (src/dcop.jl:53-94).
    if (r == 1 && S > 1) {
      for (int c = 0; c < A.n_comp; ++c) {
        int donor = -1;
        for (int s = 0; s < S && donor < 0; ++s) if (!active[(size_t)c * S + s] && donor_ok[(size_t)c * S + s]) donor = s;
        if (donor < 0) continue;
        for (int s = 0; s < S; ++s) if (active[(size_t)c * S + s])
          for (int u = A.comp_uofs[c]; u < A.comp_uofs[c] + A.comp_nc[c]; ++u) xs[(size_t)s * A.n_unk + u] = xs[(size_t)donor * A.n_unk + u];
      }
    }
  }
  // behind a pass, from `status`: converged blocks leave the active set and become donors
  void harvest() {
    n_active = 0;
    for (int b = 0; b < nblk; ++b) if (active[b]) { if (status[b] == 0) { active[b] = 0; donor_ok[b] = 1; } else ++n_active; }
  }
  // per sample: CH_OK, or what its (last) unconverged block reported
  void sample_status(std::vector<int>& out) const {
    out.assign(S, CH_OK);
    for (int b = 0; b < nblk; ++b) if (active[b]) out[b % S] = status[b] == 2 ? CH_ERR_SINGULAR : CH_ERR_MAXITERS;
  }
};

}  // namespace chip
